// gap_profile.hip.h -- one path set scored for many lengths of ONE gap (gaml_hip_gap_profile), and the gap-length search
// of the reference on top of it (gaml_hip_fix_gap_length: FixGapLength moves.cc:694-800).
// (one translation unit with gaml_hip.hip, which includes this file behind advice.hip.h)
//
// A gap's length moves every window behind the gap and changes 2T -- nothing else. Windows never span a gap
// (GetSubpathsFromPath graph.cc:495-533 ends a sub-walk there; junction() with stop_at_gap), so every candidate length
// registers and aligns the same windows; a window's filter threshold is kept relative to the window (min_pos =
// (max_pos - 5) - shift, max_pos starting again at 0 in every contig: occurrences_from_placements), so neither it nor
// the "general" flag that follows from it (occ_prepack: min_pos > 32767) moves; ranks and path slots stay. What differs
// between two candidates is the `shift` word of the occurrences of the edited path behind the gap -- in the 12-byte
// table entries and in the lists of windows that occur several times -- and the thresholds that follow from 2T.
// A set with a coverage penalty has its coverage layout [slot_base | path_base | start_off | starts] (paired_cov_build) as
// well: a path keeps bits(len) = ((len + 64 + 31) / 32) * 32 bits, so the edited path's region grows by dbits = bits(len + d)
// - bits(len) (a multiple of 32, not d), every region behind it moves by dbits, and the edited path's contig starts behind
// the gap move by d. Marks need nothing new: a lane marks at slot_base[slot] + shift + position. Such a set takes the device
// route only where the context asks for it (gaml_hip_set_gap_penalty_device / GAML_HIP_GAP_PENALTY=device).
// Single-end sets and PacBio sets without a coverage penalty go along where the context asks for that
// (gaml_hip_set_gap_mixed_device / GAML_HIP_GAP_MIXED=device; gap_mixed.hip.h): a single-end set's tables of every length are
// derived from ONE host-built table (every rank behind the gap moves, the later paths' too), a PacBio set's count columns from
// one enumeration per profile plus the sub-walks that contain the gap entry. A PacBio set WITH a penalty keeps its context
// on the fallback whatever gaml_hip_set_pacbio_penalty_onepass says: its contig sweeps would have to run per length.
//
//   gap_tables_kernel     region g of an arena slot := the resident tables, those shift words + (lens[g] - base); for a
//                         penalised set a third grid row: region g's coverage layout := the resident one by the rules above
//   gap_mixed_plan / _launch / _collect   the other kinds' side of a profile and of a pass (gap_mixed.hip.h)
//   gap_profile_device    plan the set once with the base length, then per pass of up to kMaxSets lengths: thresholds
//                         through the BAR, gap_tables_kernel, paired_score_multi_kernel (launch_paired_multi, unchanged;
//                         a penalised set: every length a PairedPrep with its own total_bits, bitmaps and sweep as a batch's);
//                         scope, wait and results of a pass are the batch routes' (MultiPass, multi_wait, multi_collect:
//                         paired_batch.hip.h), the copy geometry theirs too (paired_tab_geometry)
//   gap_profile_fallback  the same lengths as path sets of gaml_hip_calc_prob_batch / collective gaml_hip_calc_prob calls
//   gaml_hip_fix_gap_length  the search, its evaluations taken from passes of lengths chosen before they are needed
#pragma once
#include "gap_mixed.hip.h"

namespace gaml {

struct GapTabArgs {
  const char* base;      // the resident tables: the path set with the base length in the gap
  char* regions;         // set g at regions + g * stride, laid out like the resident tables
  size_t stride;
  size_t off_occ[2], bytes_occ[2], off_lo[2], bytes_lo[2], off_m[2], bytes_m[2];  // per mate; occ: multiples of 12, lists: of 4 / 16
  int n_occ[2];          // table entries that may be present (the windows there are); the copy may be longer
  int n_lists[2];        // lists of windows that occur several times, and their entries
  int n_multi[2];
  int slot;              // path slot of the edited path (what its entries carry as their path)
  int first_rank[2];     // path-local rank of the first occurrence behind the gap, per mate
  int n_sets;            // sets of this launch
  int delta[kMaxSets];   // set g: its gap length minus the base length
  unsigned char* chg[2]; // per mate: MultiSets::chg of this launch (one byte per table entry)
  size_t chg_bytes[2];   // multiples of 16, >= n_occ
  // a set with a coverage penalty (cov != 0; grid row 2): the layout [slot_base | path_base | start_off | starts] of the set
  // with the base length sits in the resident copy, every region gets its own at the same offsets
  int cov;
  size_t off_sb, off_pb, off_so, off_st;  // from `base` / from a region's start
  int n_sb, n_pb, n_st;  // slots; paths + 1 (path_base and start_off alike); contig starts of all paths
  int edited;            // position of the edited path in the set
  int edited_base;       // path_base[edited] of the base layout: a region behind it starts at a larger bit
  int st_from, st_to;    // starts[st_from .. st_to): the edited path's contig starts behind the gap
  int dbits[kMaxSets];   // set g: bits the edited path's region grows by (a multiple of 32; not delta)
};

// a direct entry {lo = shift, hi = min_pos:16 | path:15 | general:1, rank} of the edited path behind the gap
__device__ __forceinline__ bool gap_direct_behind(unsigned lo, unsigned hi, int rank, int slot, int first_rank) {
  if (lo == ~0u && hi == ~0u) return false;  // the window does not occur
  if (hi >> 31) return false;                // its occurrences are in a list
  return (int)((hi >> 16) & 0x7fffu) == slot && rank >= first_rank;
}

// grid (sets of this launch + 1, 2 mates), and a third row when the set carries a coverage penalty
__global__ __launch_bounds__(1024) void gap_tables_kernel(GapTabArgs a) {
  if (blockIdx.y == 2) {
    // region g's coverage layout (paired_cov_build of the set planned with lens[g]): the edited path's region grows by
    // dbits, every region behind it moves by as much, the edited path's contig starts behind the gap move by delta
    const int g = (int)blockIdx.x;
    if (g >= a.n_sets) return;
    const int delta = a.delta[g], dbits = a.dbits[g];
    char* region = a.regions + (size_t)g * a.stride;
    const int* src_sb = (const int*)(a.base + a.off_sb);
    const int* src_pb = (const int*)(a.base + a.off_pb);
    const int* src_so = (const int*)(a.base + a.off_so);
    const int* src_st = (const int*)(a.base + a.off_st);
    int* dst_sb = (int*)(region + a.off_sb);
    int* dst_pb = (int*)(region + a.off_pb);
    int* dst_so = (int*)(region + a.off_so);
    int* dst_st = (int*)(region + a.off_st);
    for (int j = (int)threadIdx.x; j < a.n_sb; j += (int)blockDim.x) { const int v = src_sb[j]; dst_sb[j] = v + (v > a.edited_base ? dbits : 0); }
    for (int j = (int)threadIdx.x; j < a.n_pb; j += (int)blockDim.x) { dst_pb[j] = src_pb[j] + (j > a.edited ? dbits : 0); dst_so[j] = src_so[j]; }
    for (int j = (int)threadIdx.x; j < a.n_st; j += (int)blockDim.x) dst_st[j] = src_st[j] + (j >= a.st_from && j < a.st_to ? delta : 0);
    return;
  }
  const int mt = (int)blockIdx.y;
  const int* src_occ = (const int*)(a.base + a.off_occ[mt]);
  const int* src_lo = (const int*)(a.base + a.off_lo[mt]);
  const int4* src_m = (const int4*)(a.base + a.off_m[mt]);
  if ((int)blockIdx.x == a.n_sets) {
    if (a.cov) return;  // (a penalised launch runs without the capture: launch_paired_multi)
    // which entries differ between the sets of this launch: every shifted one, in every set behind the first (the
    // lengths of a launch are distinct; equal ones would only resolve a pair again). A thread writes four entries' bytes.
    const unsigned bits = (0xfeu & ((1u << a.n_sets) - 1u));
    unsigned* out = (unsigned*)a.chg[mt];
    for (size_t t = threadIdx.x; t < a.chg_bytes[mt] / 4; t += blockDim.x) {
      unsigned word = 0;
      for (int k = 0; k < 4; k++) {
        const size_t w = 4 * t + k;
        if (w >= (size_t)a.n_occ[mt]) break;
        const unsigned lo = (unsigned)src_occ[3 * w], hi = (unsigned)src_occ[3 * w + 1];
        const int rank = src_occ[3 * w + 2];
        bool moved = gap_direct_behind(lo, hi, rank, a.slot, a.first_rank[mt]);
        if (!moved && !(lo == ~0u && hi == ~0u) && (hi >> 31)) {
          const int list = -rank - 1;
          if (list >= 0 && list < a.n_lists[mt]) {
            int q0 = src_lo[list], q1 = src_lo[list + 1];
            if (q0 < 0) q0 = 0;
            if (q1 > a.n_multi[mt]) q1 = a.n_multi[mt];
            for (int q = q0; q < q1 && !moved; q++) { const int4 e = src_m[q]; moved = e.z == a.slot && e.w >= a.first_rank[mt]; }
          }
        }
        if (moved) word |= bits << (8 * k);
      }
      out[t] = word;
    }
    return;
  }
  const int g = (int)blockIdx.x;
  const int delta = a.delta[g];
  char* region = a.regions + (size_t)g * a.stride;
  int* dst_occ = (int*)(region + a.off_occ[mt]);
  const size_t words = a.bytes_occ[mt] / 4, live = 3 * (size_t)a.n_occ[mt];
  for (size_t j = threadIdx.x; j < words; j += blockDim.x) {
    int v = src_occ[j];
    if (delta != 0 && j < live && j % 3 == 0 && gap_direct_behind((unsigned)v, (unsigned)src_occ[j + 1], src_occ[j + 2], a.slot, a.first_rank[mt])) v += delta;
    dst_occ[j] = v;
  }
  block_copy_words(region + a.off_lo[mt], a.base + a.off_lo[mt], a.bytes_lo[mt]);
  int4* dst_m = (int4*)(region + a.off_m[mt]);
  for (size_t q = threadIdx.x; q < a.bytes_m[mt] / 16; q += blockDim.x) {
    int4 e = src_m[q];  // OccQuad {shift, min_pos, path, rank}
    if (q < (size_t)a.n_multi[mt] && e.z == a.slot && e.w >= a.first_rank[mt]) e.x += delta;
    dst_m[q] = e;
  }
}

}  // namespace gaml

namespace {

// may this context take the device route at all (what does not depend on the path set)
bool gap_device_capable(const gaml_hip_ctx* c) {
  if (c->multi || c->comm || c->device < 0 || c->world != 1 || c->peers != 1) return false;
  if (KNOB(c, GAP_FALLBACK) == 1) return false;  // the fallback route (A/B, tests)
  if (!c->direct_write || KNOB(c, UPLOAD_ROUTE) != 0 || KNOB(c, NO_RESIDENT_TABLES) != 0) return false;
  // a set with a coverage penalty: gap_tables_kernel derives every length's coverage layout too, where the context asks for it
  // (gaml_hip_set_gap_penalty_device); otherwise such a context searches through the fallback (whose multi-length steps are
  // batches, one pass each)
  if (!c->gap_penalty_device) for (auto& ps : c->paireds) if (ps->cfg.penalty_constant > 0) return false;
  bool others = false;
  for (auto& h : c->handles) if (h.kind != 1) others = true;
  if (!others) return batch_fast_capable(c);
  // single-end and PacBio sets: their tables and count columns are derived per pass too (gap_mixed.hip.h), where the context
  // asks for it (gaml_hip_set_gap_mixed_device). A PacBio set with a coverage penalty stays on the fallback whatever
  // gaml_hip_set_pacbio_penalty_onepass says: every length would need the contig sweeps of its own coordinates. The route
  // launches single_score_multi_kernel itself: gaml_hip_set_single_onepass, which governs batches, is not asked.
  if (!c->gap_mixed_device) return false;
  for (auto& pb : c->pacbios) if (pb->cfg.penalty_constant > 0) return false;
  if (KNOB(c, BATCH_ROUTE) == GAML_HIP_BATCH_SEQUENTIAL) return false;
  for (auto& ps : c->paireds) if (!paired_multi_capable(c, *ps)) return false;
  return true;
}

// The device route. c->gap_flat / gap_offs hold the path set with `base_len` in the gap. Returns 1 when the set cannot go
// this way (the caller takes the fallback), < 0 on an error.
int gap_profile_device(gaml_hip_ctx* c, int32_t n_paths, int32_t path_id, int32_t gap_pos, int32_t base_len, const int32_t* lens,
                       int32_t n_lens, double* probs_out, int32_t* zeros_out, int32_t* tls_out) {
  hipStream_t st = c->stream;
  const size_t nps = c->paireds.size();
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto& ps : c->paireds) paired_images_refresh(*ps);
  // penalised sets: a path keeps bits(len) bits of the coverage bitmap (paired_cov_build), so a length moves the set's
  // total_bits by dbits = bits(len + d) - bits(len) of the edited path; every length's total must fit int32
  bool any_cov = false;
  for (auto& ps : c->paireds) any_cov = any_cov || ps->cfg.penalty_constant > 0;
  auto cov_bits_of = [](int64_t len) { return ((len + 64 + 31) / 32) * 32; };
  int64_t edited_len = 0, base_bits = 0;
  int starts_before = 1;  // contig starts of the edited path that are not behind the gap: the path's own and one per gap in front
  if (any_cov) {
    for (int32_t k = 0; k < n_paths; k++) {
      int64_t len = 0;
      for (int64_t q = c->gap_offs[k]; q < c->gap_offs[k + 1]; q++) len += c->gap_flat[q] < 0 ? -(int64_t)c->gap_flat[q] : c->g.len(c->gap_flat[q]);
      if (k == path_id) edited_len = len;
      base_bits += cov_bits_of(len);
    }
    for (int64_t q = c->gap_offs[path_id]; q < c->gap_offs[path_id] + gap_pos; q++) if (c->gap_flat[q] < 0) starts_before++;
    for (int32_t k = 0; k < n_lens; k++)
      if (base_bits + cov_bits_of(edited_len + (lens[k] - base_len)) - cov_bits_of(edited_len) > 0x7fffffffLL) return 1;  // (the fallback says what is wrong)
    for (auto& ps : c->paireds) ps->batch_bad.clear();  // per length of this profile (multi_collect)
  }
  struct PerSet {
    int slot = 0; char* wp = nullptr; size_t stride = 0;
    PairedLayout L; std::vector<PairedLayout> Ls; std::vector<PairedPrep> prep;
    size_t bw[2] = {0, 0}, chg_bytes[2] = {0, 0};
    int path_slot = 0, first_rank[2] = {0, 0};
    bool cov = false; int32_t base_bits = 0; int st_from = 0, st_to = 0, edited_base = 0;
  };
  std::vector<PerSet> per(nps);
  const int chunk = std::min<int32_t>(kMaxSets, n_lens);
  MultiPass pass(c, chunk);  // (every pass of `chunk` lengths goes out in one launch: nothing to plan beside it)
  for (size_t i = 0; i < nps; i++) { if (int e = prepare_paired_tables(c, *c->paireds[i])) return e; }
  int64_t pending = 0;
  if (int e = eval_begin(c, c->gap_flat.data(), c->gap_offs.data(), n_paths, &pending)) return e;
  const int32_t tl0 = c->pending_total_len;
  // where the gap starts in the path: every occurrence in front of it starts before that coordinate + the base length
  // (an occurrence's shift is where its node starts), every one behind it at or after
  int64_t gap_from = 0;
  for (int64_t q = c->gap_offs[path_id]; q < c->gap_offs[path_id] + gap_pos; q++) gap_from += c->gap_flat[q] < 0 ? -(int64_t)c->gap_flat[q] : c->g.len(c->gap_flat[q]);
  for (size_t i = 0; i < nps; i++) {
    PairedSet& ps = *c->paireds[i];
    PerSet& r = per[i];
    r.prep.resize(1);
    if (int e = prepare_paired_tables_host(c, ps, r.prep[0])) return e;
    if (int e = paired_sync_tables(c, ps, st)) return e;
    PairedSet::Persist& P = ps.persist;
    // the resident copy follows the images: now the set with the base length -- of a penalised set with its coverage layout
    r.cov = ps.cfg.penalty_constant > 0;
    PairedLayout cov_L;
    memset(&cov_L, 0, sizeof(cov_L));
    if (r.cov) { if (int e = paired_persist_update(c, ps, (double)(2 * (tl0 == 0 ? 1 : tl0)), st, &r.prep[0], &cov_L)) return e; }
    else if (paired_persist_stale(ps)) { if (int e = paired_persist_update(c, ps, (double)(2 * (tl0 == 0 ? 1 : tl0)), st)) return e; }
    if ((size_t)path_id >= ps.planner.slots().size()) return fail(c, GAML_HIP_ESTATE, "gap profile: the planner does not hold the path set");
    r.path_slot = ps.planner.slots()[(size_t)path_id];
    const PathMemo& pm = ps.planner.memo(ps.planner.ids()[(size_t)path_id]);
    for (int mt = 0; mt < 2; mt++) {
      int k = 0;
      for (const Occ& o : pm.occ[mt]) if ((int64_t)o.shift < gap_from + base_len) k++;
      r.first_rank[mt] = k;
      r.bw[mt] = std::max<size_t>(std::max<size_t>(1, ps.image[mt].occ12.size()), ps.mate[mt].wins.size());  // (a record's window id indexes the tables and the chg bytes)
      if (r.bw[mt] > P.cap_w[mt] || ps.image[mt].multi_off.size() > P.cap_lo[mt] || ps.image[mt].multi.size() > P.cap_m[mt]) return 1;  // (the update above made room: cannot happen)
      r.chg_bytes[mt] = align16(r.bw[mt]);
    }
    r.stride = align16(P.blk.cap);
    r.L = paired_persist_layout(P);
    if (r.cov) {
      const PairedPrep& p0 = r.prep[0];
      if ((size_t)path_id + 1 >= p0.path_base.size() || (int64_t)p0.total_bits != base_bits) return fail(c, GAML_HIP_ESTATE, "gap profile: the coverage layout is not the path set's");
      r.L.sb_off = cov_L.sb_off; r.L.pb_off = cov_L.pb_off; r.L.so_off = cov_L.so_off; r.L.st_off = cov_L.st_off;  // (every region: at the resident copy's offsets)
      r.base_bits = p0.total_bits;
      r.edited_base = p0.path_base[(size_t)path_id];
      r.st_from = std::min(p0.start_off[(size_t)path_id] + starts_before, p0.start_off[(size_t)path_id + 1]);
      r.st_to = p0.start_off[(size_t)path_id + 1];
    }
    r.Ls.assign((size_t)chunk, r.L);
    { const PairedPrep one = r.prep[0]; r.prep.assign((size_t)chunk, one); }  // every length: the same windows, lists and records
    if (int e = arena_acquire(c, ps.arena, r.stride * (size_t)chunk + r.chg_bytes[0] + r.chg_bytes[1], st, &r.slot, &r.wp)) return e;
  }
  // the sets of the other kinds (none unless gaml_hip_set_gap_mixed_device let the context in): one host table / one
  // enumeration per profile; a set that cannot go hands the profile to the fallback before anything reached its bookkeeping
  GapMixed mixed(c);
  if (int e = gap_mixed_plan(c, mixed, path_id, gap_pos, base_len, chunk, st)) return e;
  c->pending_open = false;
  const size_t ns = std::max<size_t>(1, c->handles.size());
  std::vector<double> part((size_t)kMaxSets * 4 * ns);
  for (int32_t done = 0; done < n_lens;) {
    const int n = std::min<int32_t>(chunk, n_lens - done);
    int32_t tls[kMaxSets];
    for (int k = 0; k < n; k++) tls[k] = tl0 + (lens[done + k] - base_len);  // (the caller checked that every total fits)
    if (int e = gap_mixed_launch(c, mixed, lens + done, n, st)) return e;  // (before the paired sets' work, as batch_chunk_patched orders them)
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      PerSet& r = per[i];
      for (int k = 0; k < n; k++) paired_pack_thresholds(ps, r.L.tfloor_off, (double)(2 * (tls[k] == 0 ? 1 : tls[k])), r.wp + (size_t)k * r.stride);
      if (int e = arena_commit(c, ps.arena, r.slot, 0, st)) return e;  // (direct route: drains the write-combining buffers)
      GapTabArgs ta;
      memset(&ta, 0, sizeof(ta));
      paired_tab_geometry(ta, ps, ps.arena.slot[r.slot].dev, r.stride, r.bw, (unsigned char*)ps.arena.slot[r.slot].dev + r.stride * (size_t)chunk, r.chg_bytes);
      for (int mt = 0; mt < 2; mt++) {
        ta.n_occ[mt] = (int)ps.image[mt].occ12.size();
        ta.n_lists[mt] = ps.image[mt].multi_off.empty() ? 0 : (int)ps.image[mt].multi_off.size() - 1;
        ta.n_multi[mt] = (int)ps.image[mt].multi.size();
        ta.first_rank[mt] = r.first_rank[mt];
      }
      ta.slot = r.path_slot;
      ta.n_sets = n;
      for (int k = 0; k < n; k++) ta.delta[k] = lens[done + k] - base_len;
      if (r.cov) {
        const PairedPrep& p0 = r.prep[0];
        ta.cov = 1;
        ta.off_sb = r.L.sb_off; ta.off_pb = r.L.pb_off; ta.off_so = r.L.so_off; ta.off_st = r.L.st_off;
        ta.n_sb = (int)p0.slot_base.size(); ta.n_pb = (int)p0.path_base.size(); ta.n_st = (int)p0.starts.size();
        ta.edited = path_id; ta.edited_base = r.edited_base;
        ta.st_from = r.st_from; ta.st_to = r.st_to;
        for (int k = 0; k < n; k++) {
          ta.dbits[k] = (int)(cov_bits_of(edited_len + ta.delta[k]) - cov_bits_of(edited_len));
          r.prep[(size_t)k].total_bits = r.base_bits + ta.dbits[k];  // (launch_paired_multi sizes the bitmaps and the sweep from it)
        }
        ps.gap_cov = PairedSet::GapCov{r.slot, n, r.stride, r.L.sb_off, r.L.pb_off, r.L.so_off, r.L.st_off, ta.n_sb, ta.n_pb, ta.n_st, {0}};
        for (int k = 0; k < n; k++) ps.gap_cov.total_bits[k] = r.prep[(size_t)k].total_bits;
      }
      hipLaunchKernelGGL(gap_tables_kernel, dim3((unsigned)n + 1, r.cov ? 3 : 2), dim3(1024), 0, st, ta);
      HIP_TRY(c, hipGetLastError());
      const unsigned char* chg[2] = {ta.chg[0], ta.chg[1]};
      if (int e = launch_paired_multi(c, ps, 0, n, r.Ls.data(), r.prep.data(), tls, (const char*)ps.arena.slot[r.slot].dev, r.stride, st, chg)) return e;
    }
    if (int e = multi_wait(c)) return e;
    multi_collect(c, n, part.data(), any_cov);
    gap_mixed_collect(c, mixed, n, lens[done + n - 1], part.data());
    for (int k = 0; k < n; k++) {
      const int32_t at = done + k;
      if (int e = combine(c, part.data() + (size_t)k * 4 * ns, &probs_out[at], zeros_out ? zeros_out + (size_t)at * 2 * ns : nullptr, tls[k])) return e;
      if (tls_out) tls_out[at] = tls[k];
    }
    c->gap_stats[3]++;
    done += n;
  }
  c->gap_stats[1] += n_lens;
  return 0;
}

// the path set with `len` in the gap, appended to flat / offs as one more set of a batch
void gap_append_set(const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos, int32_t len,
                    std::vector<int32_t>& flat, std::vector<int64_t>& flat_offs) {
  const int64_t base = offs[0], at = (int64_t)flat.size();
  flat.insert(flat.end(), paths + base, paths + offs[n_paths]);
  flat[(size_t)(at + offs[path_id] - base + gap_pos)] = -len;
  if (flat_offs.empty()) flat_offs.push_back(0);
  for (int32_t k = 1; k <= n_paths; k++) flat_offs.push_back(at + offs[k] - base);
}

int gap_profile_fallback(gaml_hip_ctx* c, const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos,
                         const int32_t* lens, int32_t n_lens, double* probs_out, int32_t* zeros_out, int32_t* tls_out) {
  const size_t ns = (size_t)std::max(1, gaml_hip_num_readsets(c));
  std::vector<int32_t> flat;
  std::vector<int64_t> flat_offs;
  if (c->comm && !c->multi) {  // rank-per-process: collective calls, one per length (every rank gets the same bits)
    for (int32_t k = 0; k < n_lens; k++) {
      flat.clear(); flat_offs.clear();
      gap_append_set(paths, offs, n_paths, path_id, gap_pos, lens[k], flat, flat_offs);
      if (int e = gaml_hip_calc_prob(c, flat.data(), flat_offs.data(), n_paths, &probs_out[k], zeros_out ? zeros_out + (size_t)k * 2 * ns : nullptr,
                                     tls_out ? tls_out + k : nullptr)) return e;
    }
  } else {
    std::vector<int32_t> set_offs((size_t)n_lens + 1, 0);
    for (int32_t k = 0; k < n_lens; k++) {
      gap_append_set(paths, offs, n_paths, path_id, gap_pos, lens[k], flat, flat_offs);
      set_offs[(size_t)k + 1] = (k + 1) * n_paths;
    }
    if (int e = gaml_hip_calc_prob_batch(c, n_lens, flat.data(), flat_offs.data(), set_offs.data(), probs_out, zeros_out, tls_out)) return e;
  }
  c->gap_stats[2] += n_lens;
  return 0;
}

// arguments both entry points share; *rest_out: the set's total length without the gap
int gap_check_args(gaml_hip_ctx* c, const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos, int64_t* rest_out) {
  if (!c || !paths || !offs || n_paths <= 0) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  if (path_id < 0 || path_id >= n_paths) return fail(c, GAML_HIP_EINVAL, "path_id out of range");
  for (int32_t k = 0; k < n_paths; k++) if (offs[k + 1] < offs[k]) return fail(c, GAML_HIP_EINVAL, "path offsets must not decrease");
  if (gap_pos < 0 || gap_pos >= offs[path_id + 1] - offs[path_id]) return fail(c, GAML_HIP_EINVAL, "gap_pos out of range");
  if (paths[offs[path_id] + gap_pos] >= 0) return fail(c, GAML_HIP_EINVAL, "the entry at gap_pos is not a gap");
  const int32_t n_nodes = gaml_hip_num_nodes(c);
  if (n_nodes <= 0) return fail(c, GAML_HIP_ESTATE, "no graph set");
  int64_t total = 0;
  for (int64_t q = offs[0]; q < offs[n_paths]; q++) {
    if (q == offs[path_id] + gap_pos) continue;
    const int32_t x = paths[q];
    if (x >= n_nodes) return fail(c, GAML_HIP_EINVAL, "path refers to a node outside the graph");
    total += x < 0 ? -(int64_t)x : (int64_t)(c->multi ? gaml_hip_node_len(c, x) : c->g.len(x));
  }
  *rest_out = total;
  return 0;
}

// values for `lens` (all >= 1, totals fit); base_len: the length the device route plans the set with
int gap_profile_impl(gaml_hip_ctx* c, const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos, int32_t base_len,
                     const int32_t* lens, int32_t n_lens, double* probs_out, int32_t* zeros_out, int32_t* tls_out) {
  c->gap_stats[0]++;
  if (n_lens == 0) return 0;
  if (!c->multi && !c->comm && c->device < 0) return fail(c, GAML_HIP_ENODEVICE, "scoring needs a HIP device: this context is host-only");
  if (gap_device_capable(c)) {
    c->gap_flat.clear(); c->gap_offs.clear();
    gap_append_set(paths, offs, n_paths, path_id, gap_pos, base_len, c->gap_flat, c->gap_offs);
    const int rc = gap_profile_device(c, n_paths, path_id, gap_pos, base_len, lens, n_lens, probs_out, zeros_out, tls_out);
    if (rc <= 0) return rc;
  }
  return gap_profile_fallback(c, paths, offs, n_paths, path_id, gap_pos, lens, n_lens, probs_out, zeros_out, tls_out);
}

// The values the search asks for, from passes of up to kMaxSets lengths: what is asked for now and, on the device route,
// lengths it may ask for next. A value is a function of the length alone, so one computed early is the one the
// reference would compute when it gets there.
struct GapValues {
  gaml_hip_ctx* c; const int32_t* paths; const int64_t* offs; int32_t n_paths, path_id, gap_pos, base_len; int64_t rest; bool speculate;
  std::vector<std::pair<int32_t, double>> known;
  const double* find(int64_t len) const { for (auto& kv : known) if (kv.first == len) return &kv.second; return nullptr; }
  bool fits(int64_t len) const { return len >= 1 && rest + len <= 0x7fffffffLL; }
  // need[]: lengths the search evaluates next whatever their values; maybe[]: lengths it may evaluate after them
  int get(const int64_t* need, int n_need, const int64_t* maybe, int n_maybe) {
    int32_t lens[kMaxSets];
    int n = 0;
    auto add = [&](int64_t len) { if (n < kMaxSets && !find(len) && std::find(lens, lens + n, (int32_t)len) == lens + n) lens[n++] = (int32_t)len; };
    for (int k = 0; k < n_need; k++) {
      if (!fits(need[k])) return fail(c, GAML_HIP_EINVAL, "gap length search: the total length would not fit int32");
      add(need[k]);
    }
    if (n == 0) return 0;
    if (speculate) for (int k = 0; k < n_maybe; k++) if (fits(maybe[k])) add(maybe[k]);
    double probs[kMaxSets];
    if (int e = gap_profile_impl(c, paths, offs, n_paths, path_id, gap_pos, base_len, lens, n, probs, nullptr, nullptr)) return e;
    for (int k = 0; k < n; k++) known.emplace_back(lens[k], probs[k]);
    return 0;
  }
};

// mid1 / mid2 of the ternary step on [lo, hi] (moves.cc:715-716), or for a span of 2 the one length evaluated there (:704-706)
int gap_ternary_lengths(int64_t lo, int64_t hi, int64_t* out) {
  const int64_t span = hi - lo;
  if (span <= 1) return 0;
  if (span == 2) { out[0] = lo; return 1; }
  out[0] = lo + span / 3; out[1] = lo + span / 3 * 2;
  return 2;
}

}  // namespace

extern "C" {

int gaml_hip_gap_profile(gaml_hip_ctx* c, const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos,
                         const int32_t* lens, int32_t n_lens, double* probs_out, int32_t* zeros_out, int32_t* total_lens_out) {
  int64_t rest = 0;
  if (int e = gap_check_args(c, paths, offs, n_paths, path_id, gap_pos, &rest)) return e;
  if (n_lens < 0 || (n_lens > 0 && (!lens || !probs_out))) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  for (int32_t k = 0; k < n_lens; k++) {
    if (lens[k] < 1) return fail(c, GAML_HIP_EINVAL, "gap lengths must be at least 1");
    if (rest + lens[k] > 0x7fffffffLL) return fail(c, GAML_HIP_EINVAL, "the total length would not fit int32");
  }
  return gap_profile_impl(c, paths, offs, n_paths, path_id, gap_pos, n_lens > 0 ? lens[0] : 1, lens, n_lens, probs_out, zeros_out, total_lens_out);
}

int gaml_hip_set_gap_penalty_device(gaml_hip_ctx* c, int32_t on) {
  if (!c) return GAML_HIP_EINVAL;
  c->gap_penalty_device = on != 0;  // (a context the device route never serves only keeps the flag: gap_device_capable)
  return GAML_HIP_OK;
}
int gaml_hip_get_gap_penalty_device(const gaml_hip_ctx* c) { return c && c->gap_penalty_device ? 1 : 0; }

int gaml_hip_set_gap_mixed_device(gaml_hip_ctx* c, int32_t on) {
  if (!c) return GAML_HIP_EINVAL;
  c->gap_mixed_device = on != 0;  // (a context the device route never serves only keeps the flag: gap_device_capable)
  return GAML_HIP_OK;
}
int gaml_hip_get_gap_mixed_device(const gaml_hip_ctx* c) { return c && c->gap_mixed_device ? 1 : 0; }

int gaml_hip_gap_stats(gaml_hip_ctx* c, int64_t* out4) {
  if (!c || !out4) return GAML_HIP_EINVAL;
  for (int k = 0; k < 4; k++) out4[k] = c->gap_stats[k];
  return GAML_HIP_OK;
}

int gaml_hip_fix_gap_length(gaml_hip_ctx* c, const int32_t* paths, const int64_t* offs, int32_t n_paths, int32_t path_id, int32_t gap_pos,
                            int32_t* len_out, int32_t* trace_lens, double* trace_probs, int32_t trace_cap, int32_t* n_trace_out) {
  int64_t rest = 0;
  if (int e = gap_check_args(c, paths, offs, n_paths, path_id, gap_pos, &rest)) return e;
  if (!len_out || trace_cap < 0 || (trace_cap > 0 && (!trace_lens || !trace_probs))) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const int64_t cur = -(int64_t)paths[offs[path_id] + gap_pos];
  GapValues v{c, paths, offs, n_paths, path_id, gap_pos, (int32_t)cur, rest, gap_device_capable(c), {}};
  if (!v.fits(cur + 1)) return fail(c, GAML_HIP_EINVAL, "the total length would not fit int32");  // (cur + 1 is always probed)
  if (!c->multi && !c->comm && c->device < 0) return fail(c, GAML_HIP_ENODEVICE, "scoring needs a HIP device: this context is host-only");
  int32_t n_trace = 0;
  auto note = [&](int64_t len) -> double {  // one evaluation of the reference, in its order
    const double p = *v.find(len);
    if (n_trace < trace_cap) { trace_lens[n_trace] = (int32_t)len; trace_probs[n_trace] = p; }
    n_trace++;
    return p;
  };
  auto done = [&](int64_t len) { *len_out = (int32_t)len; if (n_trace_out) *n_trace_out = n_trace; return GAML_HIP_OK; };
  // the first probes (moves.cc:740-756): cur, cur + 1 and -- unless cur is 1 -- cur - 1; beside them the bounds the way up
  // would try (:764-772)
  int64_t need[4] = {cur, cur + 1, cur - 1, 0}, maybe[kMaxSets];
  for (int k = 0; k < 5; k++) maybe[k] = cur << (k + 1);
  if (int e = v.get(need, cur == 1 ? 2 : 3, maybe, 5)) return e;
  const double cur_p = note(cur), up_p = note(cur + 1);
  int state = 0;  // 0: stay, 1: up, 2: down (:739)
  if (cur == 1) { if (up_p > cur_p) state = 1; }
  else {
    const double down_p = note(cur - 1);
    if (down_p > cur_p && cur_p > up_p) state = 2;
    if (up_p > cur_p && cur_p > down_p) state = 1;
  }
  if (state == 0) return done(cur == 1 ? cur + 1 : cur - 1);  // the entry keeps the last probed length (:741-759 never restore it)
  int64_t lo = 1, hi = cur;  // down: [1, cur] (:778)
  if (state == 1) {  // the bound doubles while the value does not drop (:763-773), then [cur + 1, bound] (:775)
    double last_p = cur_p;
    int64_t bound = 2 * cur;
    for (;;) {
      need[0] = bound;
      int nm = 0;
      for (int k = 1; k < kMaxSets; k++) maybe[nm++] = bound << k;
      // (the search that follows a drop at this bound)
      nm = std::min(nm, kMaxSets - 1 - 2);
      nm += gap_ternary_lengths(cur + 1, bound, maybe + nm);
      if (int e = v.get(need, 1, maybe, nm)) return e;
      const double p = note(bound);
      if (p < last_p) break;
      last_p = p;
      bound *= 2;
    }
    lo = cur + 1; hi = bound;
  }
  for (;;) {  // the ternary search (:694-727)
    int64_t mids[2];
    const int n_mids = gap_ternary_lengths(lo, hi, mids);
    if (n_mids == 0) return done(lo);  // (:697-700)
    // this level's lengths, and those of both levels that may follow
    int nm = 0;
    if (n_mids == 2) { nm += gap_ternary_lengths(lo, mids[1], maybe + nm); nm += gap_ternary_lengths(mids[0], hi, maybe + nm); }
    if (int e = v.get(mids, n_mids, maybe, nm)) return e;
    if (n_mids == 1) { note(lo); note(lo); return done(lo); }  // a span of 2 evaluates the lower end twice and keeps it (:702-712)
    const double p1 = note(mids[0]), p2 = note(mids[1]);
    if (p1 >= p2) hi = mids[1]; else lo = mids[0];  // (:722-726)
  }
}

}  // extern "C"
