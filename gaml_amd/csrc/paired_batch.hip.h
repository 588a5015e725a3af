// paired_batch.hip.h -- gaml_hip_calc_prob_batch over paired, PacBio and (opt-in) single-end sets: per-set tables from patches / whole, one pass over the records
// (one translation unit with gaml_hip.hip, which includes this file at the place its contents used to stand)
//
//   batch_fast_capable    may this context's batches take the one-pass routes at all
//   MultiPass, multi_wait / _drain / _collect   the frame of a multi-set pass: blocking scope, two-launch pacing, the wait,
//                         the hand-over with launches in flight, the results -- shared with gap_profile_device
//   batch_chunk_patched   a chunk of up to kMaxSets sets, their tables built on the device from the resident copy + patches
//   batch_chunk_fast      the same with whole tables per set, written by the host (takes over when patches do not do)
#pragma once

// ---------------------------------------------------------------------------------------------------------
// gaml_hip_calc_prob_batch, fast path: up to kMaxSets path sets in ONE pass over the records of every paired set
// (paired_score_multi_kernel). The host plans the sets one after the other straight into consecutive regions of one
// arena slot; then one launch per read set, one wait. Contexts with single-end sets (switch off) or without a memo take the
// sequential path of gaml_hip_calc_prob_batch (same results). A set with a coverage penalty goes along: its path sets mark into bitmaps of their
// own, one sweep dispatch per launch (launch_paired_multi); the wait is then a real stream wait, one per chunk.
// PacBio sets without a coverage penalty go along as well, beside the paired sets or on their own: one dispatch of
// pacbio_score_multi_kernel per set and chunk, enqueued before the paired sets are planned (pacbio_batch.hip.h); the wait is
// a stream wait then too. A PacBio set with a penalty keeps the whole context on the sequential path, unless the context's
// switch is on (gaml_hip_set_pacbio_penalty_onepass, off by default): then the chunk sweeps the paths it has no bad_bases
// for yet, one contig per block, behind that dispatch, and a set's bad_bases is the sum over its paths (pacbio_batch.hip.h).
// A single-end set keeps the context sequential as well, unless the context's switch is on (gaml_hip_set_single_onepass, off by default): then single-end sets go along the
// same way, one dispatch of single_score_multi_kernel per set and chunk, enqueued behind the PacBio one (single_batch.hip.h).
// ---------------------------------------------------------------------------------------------------------
static bool batch_fast_capable(const gaml_hip_ctx* c) {
  if (c->handles.empty() || KNOB(c, BATCH_ROUTE) == GAML_HIP_BATCH_SEQUENTIAL) return false;  // force the sequential path (A/B, tools/)
  if (!c->single_onepass) for (auto& h : c->handles) if (h.kind == 0) return false;  // single-end sets go along only where the context says so (single_batch.hip.h)
  if (!c->pacbio_penalty_onepass) for (auto& pb : c->pacbios) if (pb->cfg.penalty_constant > 0) return false;  // ... and so do penalised PacBio sets (pacbio_batch.hip.h)
  for (auto& ps : c->paireds) if (!paired_multi_capable(c, *ps)) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// The frame of a multi-set pass, shared by the routes that feed paired_score_multi_kernel: batch_chunk_patched and
// batch_chunk_fast below, gap_profile_device (gap_profile.hip.h). A route says how its regions are sized, what it writes
// per set, which table kernel it launches and when it gives up; the rest is here.
// ---------------------------------------------------------------------------------------------------------
// The blocking scope (results in pinned host memory; on every way out the context is as a blocking call leaves it), and
// the pacing of the two batch routes: a chunk of more than 4 sets goes out in two launches, the host plans the second
// half while the device scores the first.
struct MultiPass {
  gaml_hip_ctx* c;
  int n, half, launched = 0;  // (where the batch is cut makes no measurable difference: 13.1-14.8 us per set for 1+7 .. 6+2)
  MultiPass(gaml_hip_ctx* ctx, int n_sets) : c(ctx), n(n_sets), half(n_sets > 4 ? (n_sets + 1) / 2 : n_sets) { c->host_results = true; }
  ~MultiPass() { c->host_results = false; c->pending_open = false; }
  MultiPass(const MultiPass&) = delete;
  bool due(int k) const { return k + 1 == half || k + 1 == n; }  // set k is planned: sets [launched, k + 1) go out now
};

// every launch of the pass has landed (spinning on the partials where that is safe), the delta lists' counts are exact
static int multi_wait(gaml_hip_ctx* c) {
  bool spun = false;
  if (int e = wait_host_partials(c, &spun)) return e;
  if (!spun) { if (int e = collect_events(c)) return e; }
  return paired_counts_after_wait(c);
}
// best effort, before a route hands its chunk on with launches in flight (the route that takes over reports what is wrong)
static void multi_drain(gaml_hip_ctx* c) {
  bool spun = false;
  (void)wait_host_partials(c, &spun);
  if (!spun) (void)collect_events(c);
}

// after multi_wait: out[(k * read sets + slot) * 4 ..] = {sum, floored, bad bases, reads} of set k, added up in the finisher
// kernel's order from the set's stripe of pinned partials; slot: where combine() expects the read set (scoring_order). The
// slots of PacBio sets are pacbio_chunk_collect's. record_bad: the penalised sets' counters (handed over behind
// the partials, store_bad_multi_kernel) and the batch's bookkeeping of them; a pass without penalised sets leaves both alone.
static void multi_collect(gaml_hip_ctx* c, int n, double* partials_out, bool record_bad) {
  const size_t nps = c->paireds.size(), ns = c->handles.size();
  const std::vector<int> slot = slots_of_kind(c, 1);
  for (int k = 0; k < n; k++)
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      double* out = partials_out + ((size_t)k * ns + (size_t)slot[i]) * 4;
      out[0] = out[1] = out[2] = 0;
      if (ps.last_blocks[k] > 0)
        finisher_order_sum((const double*)ps.h_part_sum.p + (size_t)k * ps.host_part_stride, (const int*)ps.h_part_zero.p + (size_t)k * ps.host_part_stride,
                           ps.last_blocks[k], &out[0], &out[1]);
      out[3] = (double)ps.mate[0].n_local();
      if (record_bad) {
        if (ps.cfg.penalty_constant > 0 && ps.last_blocks[k] > 0) out[2] = (double)((const unsigned long long*)ps.h_bad.p)[k];
        ps.batch_bad.push_back((int64_t)out[2]);
      }
      ps.last_bad_bases = (int64_t)out[2];
    }
}

// A chunk with the sets' tables built on the device (batch_tables_kernel): on a large-BAR device the resident copy
// of the tables mirrors the previous call's path set, and candidates differ from it -- and from each other -- in a
// few dozen entries. Returns 1 when this chunk cannot go that way (tables rebuilt as a whole, list changes, growth
// past the resident capacities): the caller takes the full-tables route, which plans the chunk again.
static int batch_chunk_patched(gaml_hip_ctx* c, int n, const int32_t* paths, const int64_t* offs, const int32_t* set_offs,
                               double* partials_out, int32_t* tls) {
  hipStream_t st = c->stream;
  const size_t nps = c->paireds.size();
  if (!c->direct_write || KNOB(c, UPLOAD_ROUTE) != 0 || KNOB(c, NO_RESIDENT_TABLES) != 0 || KNOB(c, BATCH_ROUTE) == GAML_HIP_BATCH_FULL_TABLES) return 1;  // full tables per set (A/B)
  constexpr size_t kPatchCap = 8192;  // entries per read set and batch
  struct PerSet {
    int slot = 0; char* wp = nullptr; size_t stride = 0;
    PairedLayout L; std::vector<PairedLayout> Ls; std::vector<PairedPrep> prep;
    std::vector<int> patch_off; size_t n_patches = 0;
    size_t tail_fixed = 0, chg_bytes[2] = {0, 0};
    size_t cov_at = 0, cov_cap = 0;  // a penalised set: every region carries its set's coverage layout behind the tables, room for cov_cap ints
    size_t bw[2] = {0, 0};  // table entries per mate the batch's regions carry: the windows there are + room for those the batch itself adds (the resident copy's capacity is far larger)
    int launches = 0;
    std::vector<int32_t> touched[2];  // union of the changed entries: the resident copy follows after the batch
  };
  std::vector<PerSet> per(nps);
  MultiPass pass(c, n);
  for (size_t i = 0; i < nps; i++) {
    PairedSet& ps = *c->paireds[i];
    if (int e = prepare_paired_tables(c, ps)) return e;
    PairedSet::Persist& P = ps.persist;
    // bring the copy up to the images (made here if no blocking call has yet; entries changed by a call that did not go through it)
    if (paired_persist_stale(ps)) { if (int e = paired_persist_update(c, ps, 2.0, st)) return e; }
    PerSet& r = per[i];
    r.stride = align16(P.blk.cap);
    if (ps.cfg.penalty_constant > 0) {
      // the layout [slot_base | path_base | start_off | starts] of the largest set (paired_cov_ints: slots there are or the batch
      // may add, paths, one start per path entry at most), written through the BAR like the thresholds
      size_t most = 0, all_paths = 0;
      for (int k = 0; k < n; k++) {
        const size_t np = (size_t)(set_offs[k + 1] - set_offs[k]);
        const size_t entries = (size_t)(offs[set_offs[k + 1]] - offs[set_offs[k]]);
        most = std::max(most, 2 * (np + 1) + entries + np);
        all_paths += np;
      }
      r.cov_at = r.stride;
      r.cov_cap = (size_t)std::max(1, ps.planner.slot_count()) + all_paths + most + 16;
      r.stride = align16(r.cov_at + r.cov_cap * sizeof(int32_t));
    }
    r.L = paired_persist_layout(P);
    r.Ls.assign((size_t)n, r.L);
    r.prep.resize((size_t)n);
    r.patch_off.assign(2 * (size_t)n + 1, 0);
    // behind the regions: the patches, their offsets, and per launch and mate one byte per table entry (MultiSets::chg)
    for (int mt = 0; mt < 2; mt++) r.bw[mt] = std::min<size_t>(P.cap_w[mt], ps.image[mt].occ12.size() + 8192);
    r.chg_bytes[0] = align16(r.bw[0]); r.chg_bytes[1] = align16(r.bw[1]);
    r.tail_fixed = align16(kPatchCap * sizeof(BatchPatch)) + align16((2 * (size_t)kMaxSets + 1) * sizeof(int));
    const size_t bytes = r.stride * (size_t)n + r.tail_fixed + 2 * (r.chg_bytes[0] + r.chg_bytes[1]);
    if (int e = arena_acquire(c, ps.arena, bytes, st, &r.slot, &r.wp)) return e;
  }
  auto give_up = [&]() -> int {  // the resident copies no longer mirror the images: rewritten as a whole next time
    for (size_t i = 0; i < nps; i++) c->paireds[i]->persist.valid = false;
    if (pass.launched > 0) multi_drain(c);
    return 1;
  };
  auto launch_sets = [&](int first, int upto) -> int {
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      PerSet& r = per[i];
      if (int e = paired_sync_tables(c, ps, st)) return e;
      for (int k = first; k < upto; k++) paired_pack_thresholds(ps, r.L.tfloor_off, (double)(2 * (tls[k] == 0 ? 1 : tls[k])), r.wp + (size_t)k * r.stride);
      char* tail = r.wp + r.stride * (size_t)n;
      int* d_off = (int*)(tail + align16(kPatchCap * sizeof(BatchPatch)));
      memcpy(d_off, r.patch_off.data(), (2 * (size_t)upto + 1) * sizeof(int));
      if (int e = arena_commit(c, ps.arena, r.slot, 0, st)) return e;  // (direct route: drains the write-combining buffers)
      BatchTabArgs ta;
      char* dev_tail = (char*)ps.arena.slot[r.slot].dev + r.stride * (size_t)n;
      paired_tab_geometry(ta, ps, ps.arena.slot[r.slot].dev, r.stride, r.bw,
                          (unsigned char*)dev_tail + r.tail_fixed + (size_t)(r.launches & 1) * (r.chg_bytes[0] + r.chg_bytes[1]), r.chg_bytes);  // (the other launch's may still be read)
      ta.patches = (const BatchPatch*)dev_tail;
      ta.patch_off = (const int*)(dev_tail + align16(kPatchCap * sizeof(BatchPatch)));
      ta.first = first;
      ta.n_sets = upto - first;
      r.launches++;
      hipLaunchKernelGGL(batch_tables_kernel, dim3((unsigned)(upto - first) + 1, 2), dim3(1024), 0, st, ta);
      HIP_TRY(c, hipGetLastError());
      const unsigned char* chg[2] = {ta.chg[0], ta.chg[1]};
      if (int e = launch_paired_multi(c, ps, first, upto - first, r.Ls.data(), r.prep.data(), tls, (const char*)ps.arena.slot[r.slot].dev, r.stride, st,
                                      KNOB(c, BATCH_ROUTE) == GAML_HIP_BATCH_NO_CAPTURE ? nullptr : chg)) return e;  // every set resolves every pair (A/B)
    }
    return 0;
  };
  PbChunk pb(c);
  if (int e = pacbio_chunk_launch(c, pb, n, paths, offs, set_offs)) return e;
  SgChunk sg(c);
  if (int e = single_chunk_launch(c, sg, n, paths, offs, set_offs)) return e;
  for (int k = 0; k < n; k++) {
    int64_t pending = 0;
    if (int e = eval_begin(c, paths, offs + set_offs[k], set_offs[k + 1] - set_offs[k], &pending)) return e;
    tls[k] = c->pending_total_len;
    // pass 2 of EVERY read set before any of them may give the chunk up: eval_begin has diffed all planners against this set,
    // and a planner left without its apply() would hand the route that takes over a diff its images never saw
    for (size_t i = 0; i < nps; i++) prepare_paired_tables_host(c, *c->paireds[i], per[i].prep[(size_t)k]);
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      PerSet& r = per[i];
      const PairedSet::Persist& P = ps.persist;
      OccImage* im = ps.image;
      bool ok = !im[0].changed_all && !im[1].changed_all && !im[0].lists_changed && !im[1].lists_changed;
      for (int mt = 0; mt < 2 && ok; mt++) ok = im[mt].occ12.size() <= r.bw[mt] && r.n_patches + im[mt].changed.size() <= kPatchCap;
      if (ok && ps.cfg.penalty_constant > 0) ok = paired_cov_ints(r.prep[(size_t)k]) <= r.cov_cap;  // (the layout does not fit its room: the full-tables route)
      if (!ok) {
        if (getenv("GAML_HIP_TRACE_HOST"))
          fprintf(stderr, "batch set %d: not a patch (all %d %d, lists %d %d, windows %zu/%zu %zu/%zu, patches %zu + %zu + %zu)\n", k, (int)im[0].changed_all, (int)im[1].changed_all,
                  (int)im[0].lists_changed, (int)im[1].lists_changed, im[0].occ12.size(), P.cap_w[0], im[1].occ12.size(), P.cap_w[1], r.n_patches, im[0].changed.size(), im[1].changed.size());
        c->pending_open = false;
        return give_up();
      }
      if (ps.cfg.penalty_constant > 0) {  // this set's coverage layout into its region (fenced with the thresholds, arena_commit)
        paired_cov_layout(r.prep[(size_t)k], r.cov_at, r.Ls[(size_t)k]);
        r.Ls[(size_t)k].total = r.stride;
        paired_cov_pack(r.prep[(size_t)k], r.Ls[(size_t)k], r.wp + (size_t)k * r.stride);
      }
      BatchPatch* dp = (BatchPatch*)(r.wp + r.stride * (size_t)n);
      for (int mt = 0; mt < 2; mt++) {
        for (int32_t w : im[mt].changed) {
          const Occ12& o = im[mt].occ12[w];
          dp[r.n_patches++] = BatchPatch{w, o.lo, o.hi, o.rank};
          r.touched[mt].push_back(w);
        }
        r.patch_off[2 * (size_t)k + mt + 1] = (int)r.n_patches;
        im[mt].take_changed();
      }
    }
    c->pending_open = false;
    if (pass.due(k)) { if (int e = launch_sets(pass.launched, k + 1)) return e; pass.launched = k + 1; }
  }
  if (nps > 0 && getenv("GAML_HIP_TRACE_HOST")) {
    fprintf(stderr, "batch of %d sets, patch entries per set (mate 1 + mate 2):", n);
    for (int k = 0; k < n; k++) fprintf(stderr, " %d+%d", per[0].patch_off[2 * k + 1] - per[0].patch_off[2 * k], per[0].patch_off[2 * k + 2] - per[0].patch_off[2 * k + 1]);
    fprintf(stderr, "\n");
  }
  if (int e = multi_wait(c)) return e;
  // the device is done with the resident copies: they follow the images (now the last set's)
  for (size_t i = 0; i < nps; i++) {
    PairedSet& ps = *c->paireds[i];
    char* occ[2] = {(char*)ps.persist.blk.dev + ps.persist.off_occ[0], (char*)ps.persist.blk.dev + ps.persist.off_occ[1]};
    for (int mt = 0; mt < 2; mt++)
      for (int32_t w : per[i].touched[mt]) memcpy(occ[mt] + (size_t)w * sizeof(Occ12), &ps.image[mt].occ12[w], sizeof(Occ12));
  }
  _mm_sfence();
  for (size_t i = 0; i < nps; i++) c->paireds[i]->batches_patched++;
  multi_collect(c, n, partials_out, true);
  if (int e = pacbio_chunk_collect(c, pb, n, partials_out)) return e;
  return single_chunk_collect(c, sg, n, partials_out);
}

// A chunk with whole tables per set, packed by the host into the regions. Returns 1 when a set's tables did not fit the
// region reserved for it (the caller's sequential path takes this chunk; the region is larger next time)
static int batch_chunk_fast(gaml_hip_ctx* c, int n, const int32_t* paths, const int64_t* offs, const int32_t* set_offs,
                            double* partials_out, int32_t* tls) {
  hipStream_t st = c->stream;
  const size_t nps = c->paireds.size();
  struct PerSet { int slot = 0; char* wp = nullptr; size_t stride = 0, cap_w[2] = {0, 0}; std::vector<PairedLayout> L; std::vector<PairedPrep> prep; };
  std::vector<PerSet> per(nps);
  MultiPass pass(c, n);
  for (size_t i = 0; i < nps; i++) {
    PairedSet& ps = *c->paireds[i];
    if (int e = prepare_paired_tables(c, ps)) return e;
    // a region per path set: the occurrence images of the current window count plus room for windows and lists that
    // this very batch adds
    // windows the batch itself may add: every set's tables are padded to this many entries per mate
    per[i].cap_w[0] = ps.mate[0].wins.size() + 256 + ps.batch_slack / 24;
    per[i].cap_w[1] = ps.mate[1].wins.size() + 256 + ps.batch_slack / 24;
    const size_t lists = 2 * (sizeof(int32_t) * (ps.image[0].multi_off.size() + ps.image[1].multi_off.size()) + sizeof(OccQuad) * (ps.image[0].multi.size() + ps.image[1].multi.size()));
    const size_t est = 4096 + 12 * (per[i].cap_w[0] + per[i].cap_w[1]) + 16384 + lists + ps.batch_slack;
    per[i].stride = align16(est);
    if (int e = arena_acquire(c, ps.arena, per[i].stride * (size_t)n, st, &per[i].slot, &per[i].wp)) return e;
    per[i].L.resize((size_t)n);
    per[i].prep.resize((size_t)n);
  }
  auto launch_sets = [&](int first, int upto) -> int {
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      if (int e = paired_sync_tables(c, ps, st)) return e;
      for (int k = first; k < upto; k++) paired_pack_thresholds(ps, per[i].L[(size_t)k].tfloor_off, (double)(2 * (tls[k] == 0 ? 1 : tls[k])), per[i].wp + (size_t)k * per[i].stride);
      // (the staged route copies the regions written so far; the direct route only drains the write-combining buffers)
      if (int e = arena_commit(c, ps.arena, per[i].slot, per[i].stride * (size_t)upto, st)) return e;
      if (int e = launch_paired_multi(c, ps, first, upto - first, per[i].L.data(), per[i].prep.data(), tls, (const char*)ps.arena.slot[per[i].slot].dev, per[i].stride, st)) return e;
    }
    return 0;
  };
  PbChunk pb(c);
  if (int e = pacbio_chunk_launch(c, pb, n, paths, offs, set_offs)) return e;
  SgChunk sg(c);
  if (int e = single_chunk_launch(c, sg, n, paths, offs, set_offs)) return e;
  for (int k = 0; k < n; k++) {
    int64_t pending = 0;
    if (int e = eval_begin(c, paths, offs + set_offs[k], set_offs[k + 1] - set_offs[k], &pending)) return e;
    tls[k] = c->pending_total_len;
    for (size_t i = 0; i < nps; i++) prepare_paired_tables_host(c, *c->paireds[i], per[i].prep[(size_t)k]);  // (all of them first: see batch_chunk_patched)
    for (size_t i = 0; i < nps; i++) {
      PairedSet& ps = *c->paireds[i];
      PairedPrep& p = per[i].prep[(size_t)k];
      bool fits = ps.mate[0].wins.size() <= per[i].cap_w[0] && ps.mate[1].wins.size() <= per[i].cap_w[1];
      if (fits) { per[i].L[(size_t)k] = paired_layout(ps, p, per[i].cap_w); fits = per[i].L[(size_t)k].total <= per[i].stride; }
      if (!fits) {  // the tables outgrew the region reserved per set: the sequential path takes this chunk (after what is in flight)
        ps.batch_slack += 24 * 16384 + 2 * per[i].stride;
        if (pass.launched > 0) multi_drain(c);
        return 1;
      }
      paired_pack(ps, p, per[i].L[(size_t)k], per[i].wp + (size_t)k * per[i].stride);
    }
    c->pending_open = false;
    if (pass.due(k)) { if (int e = launch_sets(pass.launched, k + 1)) return e; pass.launched = k + 1; }
  }
  if (int e = multi_wait(c)) return e;
  for (size_t i = 0; i < nps; i++) c->paireds[i]->batches_full++;
  multi_collect(c, n, partials_out, true);
  if (int e = pacbio_chunk_collect(c, pb, n, partials_out)) return e;
  return single_chunk_collect(c, sg, n, partials_out);
}

