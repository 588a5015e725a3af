// debug_api.hip.h -- the gaml_hip_debug_* entry points (include/gaml_hip_debug.h): development builds only (-DGAML_HIP_DEV)
// (one translation unit with gaml_hip.hip, which includes this file at the place its contents used to stand)
#pragma once

int gaml_hip_debug_prepare(gaml_hip_ctx* c, const int32_t* flat, const int64_t* offs, int32_t n_paths) {
  if (!c || n_paths < 0 || (n_paths > 0 && (!flat || !offs))) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  if (c->multi) {  // every shard registers / aligns / places on its own reads (host-only shards included)
    for (int k = 0; k < gaml::multi_num_shards(c->multi); k++)
      if (int e = gaml_hip_debug_prepare(gaml::multi_shard(c->multi, k), flat, offs, n_paths)) return fail(c, e, gaml_hip_last_error(gaml::multi_shard(c->multi, k)));
    return GAML_HIP_OK;
  }
  if (!c->have_graph) return fail(c, GAML_HIP_ESTATE, "no graph set");
  std::vector<Walk> paths = unflatten(flat, offs, n_paths);
  for (auto& h : scoring_order(c)) {
    if (h.kind == 0) { std::vector<Occ> occs; int32_t tl = 0; if (int e = prepare_single_host(c, *c->singles[h.idx], paths, occs, &tl)) return e; }
    else if (h.kind == 1) {
      PairedPrep p;
      PairedSet& ps = *c->paireds[h.idx];
      if (int e = prepare_paired_structure(c, ps, flat, offs, n_paths)) return e;
      if (int e = align_pending_pair(c, ps)) return e;
      if (int e = prepare_paired_tables_host(c, ps, p)) return e;
    }
  }
  if (c->peers == 1) {
    for (ShortMate* m : filter_mates(c)) m->unsynced.clear();
  }
  return GAML_HIP_OK;
}

int64_t gaml_hip_debug_occurrences(gaml_hip_ctx* c, int rs, int mate, int32_t* out5, int64_t cap) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size()) return -1;
  SetRef h = c->handles[rs];
  const std::vector<Occ>* v = nullptr;
  if (h.kind == 0) v = &c->singles[h.idx]->last_occ;
  else if (h.kind == 1 && (mate == 0 || mate == 1)) { PairedSet& ps = *c->paireds[h.idx]; ps.planner.flat_occurrences(mate, ps.scratch_occ[mate]); v = &ps.scratch_occ[mate]; }
  if (!v) return -1;
  for (int64_t i = 0; i < (int64_t)v->size() && i < cap; i++) {
    const Occ& o = (*v)[i];
    out5[5 * i] = o.wid; out5[5 * i + 1] = o.shift; out5[5 * i + 2] = o.min_pos; out5[5 * i + 3] = o.path; out5[5 * i + 4] = o.rank;
  }
  return (int64_t)v->size();
}

int64_t gaml_hip_debug_table_occurrences(gaml_hip_ctx* c, int rs, int mate, int32_t* out5, int64_t cap, int64_t* info3) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || (mate != 0 && mate != 1)) return -1;
  PairedSet& ps = *c->paireds[c->handles[rs].idx];
  if (info3) { info3[0] = ps.planner.last_was_incremental(); info3[1] = (int64_t)ps.planner.incremental_calls; info3[2] = (int64_t)ps.planner.full_calls; }
  std::vector<Occ> v;
  paired_images_refresh(ps);
  ps.image[mate].dump(v);
  const std::vector<int32_t>& slots = ps.planner.slots();
  std::unordered_map<int32_t, int32_t> pos;
  for (size_t k = 0; k < slots.size(); k++) pos[slots[k]] = (int32_t)k;
  for (Occ& o : v) { auto it = pos.find(o.path); o.path = it == pos.end() ? -1 : it->second; }
  std::sort(v.begin(), v.end(), [](const Occ& a, const Occ& b) { return a.path != b.path ? a.path < b.path : (a.rank != b.rank ? a.rank < b.rank : a.wid < b.wid); });
  for (int64_t i = 0; i < (int64_t)v.size() && i < cap; i++) {
    const Occ& o = v[(size_t)i];
    out5[5 * i] = o.wid; out5[5 * i + 1] = o.shift; out5[5 * i + 2] = o.min_pos; out5[5 * i + 3] = o.path; out5[5 * i + 4] = o.rank;
  }
  return (int64_t)v.size();
}

int32_t gaml_hip_debug_cov_layout(gaml_hip_ctx* c, int rs, int32_t* slot_base, int32_t cap_slots, int32_t* path_base, int32_t* start_off, int32_t* slots,
                                   int32_t cap_paths, int32_t* starts, int32_t cap_starts, int32_t* counts4) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1) return -1;
  PairedSet& ps = *c->paireds[c->handles[rs].idx];
  if (!(ps.cfg.penalty_constant > 0) || ps.planner.full_calls + ps.planner.incremental_calls == 0) return -1;  // no penalty, or nothing prepared yet
  struct { std::vector<int32_t> slot_base, path_base, start_off, starts, slots; } L;
  {
    PairedPrep p;  // what pass 2 builds for the planner's current set (prepare_paired_tables_host)
    paired_cov_build(ps, true, p);
    L.slot_base.swap(p.slot_base); L.path_base.swap(p.path_base); L.start_off.swap(p.start_off); L.starts.swap(p.starts);
    L.slots = ps.planner.slots();
  }
  const int32_t n = (int32_t)L.slots.size();
  if (counts4) { counts4[0] = (int32_t)L.slot_base.size(); counts4[1] = n; counts4[2] = (int32_t)L.starts.size(); counts4[3] = L.path_base.back(); }
  for (int32_t k = 0; k < (int32_t)L.slot_base.size() && k < cap_slots; k++) slot_base[k] = L.slot_base[k];
  for (int32_t k = 0; k <= n && k <= cap_paths && cap_paths > 0; k++) { path_base[k] = L.path_base[k]; start_off[k] = L.start_off[k]; }
  for (int32_t k = 0; k < n && k < cap_paths; k++) slots[k] = L.slots[k];
  for (int32_t k = 0; k < (int32_t)L.starts.size() && k < cap_starts; k++) starts[k] = L.starts[k];
  return n;
}

int32_t gaml_hip_debug_gap_cov_layout(gaml_hip_ctx* c, int rs, int g, int32_t* slot_base, int32_t cap_slots, int32_t* path_base, int32_t* start_off,
                                       int32_t* slots, int32_t cap_paths, int32_t* starts, int32_t cap_starts, int32_t* counts4) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || c->device < 0) return -1;
  PairedSet& ps = *c->paireds[c->handles[rs].idx];
  const PairedSet::GapCov& G = ps.gap_cov;
  if (G.slot < 0 || g < 0 || g >= G.n || !ps.arena.slot[G.slot].dev) return -1;  // no device gap pass of a penalised set yet, or no such region
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  const char* region = (const char*)ps.arena.slot[G.slot].dev + (size_t)g * G.stride;
  std::vector<int32_t> sb((size_t)G.n_sb), pb((size_t)G.n_pb), so((size_t)G.n_pb), stv((size_t)std::max(1, G.n_st));
  if (hipMemcpy(sb.data(), region + G.sb_off, sb.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(pb.data(), region + G.pb_off, pb.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(so.data(), region + G.so_off, so.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (G.n_st > 0 && hipMemcpy(stv.data(), region + G.st_off, (size_t)G.n_st * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const std::vector<int32_t>& sl = ps.planner.slots();
  const int32_t n = G.n_pb - 1;
  if (counts4) { counts4[0] = G.n_sb; counts4[1] = n; counts4[2] = G.n_st; counts4[3] = G.total_bits[g]; }
  for (int32_t k = 0; k < G.n_sb && k < cap_slots; k++) slot_base[k] = sb[(size_t)k];
  for (int32_t k = 0; k <= n && k <= cap_paths && cap_paths > 0; k++) { path_base[k] = pb[(size_t)k]; start_off[k] = so[(size_t)k]; }
  for (int32_t k = 0; k < n && k < cap_paths && k < (int32_t)sl.size(); k++) slots[k] = sl[(size_t)k];
  for (int32_t k = 0; k < G.n_st && k < cap_starts; k++) starts[k] = stv[(size_t)k];
  return n;
}

int32_t gaml_hip_debug_window_walk(gaml_hip_ctx* c, int rs, int mate, int32_t wid, int32_t* out, int32_t cap) {
  MULTI_SHARD0(c);
  ShortMate* m = mate_of(c, rs, mate);
  if (!m || wid < 0 || wid >= (int32_t)m->win_walk.size()) return -1;
  const Walk& w = *m->win_walk[wid];
  for (int32_t i = 0; i < (int32_t)w.size() && i < cap; i++) out[i] = w[i];
  return (int32_t)w.size();
}



int gaml_hip_debug_timeline(gaml_hip_ctx* c, int rs, unsigned long long* out, int64_t cap_waves) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  if (!s.h_timeline.p) return 0;
  const int64_t n = std::min<int64_t>(cap_waves, s.timeline_waves);
  memcpy(out, s.h_timeline.p, (size_t)n * 8 * sizeof(unsigned long long));
  return (int)n;
}

int gaml_hip_debug_set_knob(gaml_hip_ctx* c, int knob, int value) {
  if (!c || knob < 0 || knob >= GAML_HIP_KNOB_COUNT) return GAML_HIP_EINVAL;
  if (c->multi) { for (int k = 0; k < gaml::multi_num_shards(c->multi); k++) gaml::multi_shard(c->multi, k)->knobs[knob] = value; return GAML_HIP_OK; }
  c->knobs[knob] = value;
  return GAML_HIP_OK;
}


// Host-only check of the record tables' rule "a record that is always overwritten stays out" (host_model.cc
// dominated_records) on the windows that are active now: builds the tables with and without the rule (no device) and
// verifies, record by record, that every pair's records with the rule are the records without it minus records of a
// junction window J for which the first node's own window -- active -- holds a record of the same read at the same
// position. out6 = {records left out mate 1, mate 2, pairs of the compact class with / without the rule, records
// checked, violations}. Returns GAML_HIP_ESTATE when a violation was found.
// a pair's records as the host restatement of the tables holds them (build_pair_tables)
static void paired_base_records(const PairTables& pt, int32_t slot, int mt, std::vector<RecQuad>& out) {
  const int64_t n0s = pt.class_count[0];
  if (slot < n0s) {
    const uint64_t r = pt.rec8[mt][slot];
    if (r != kNoRec8) out.push_back(RecQuad{(int32_t)(r & 0xffffff), (int32_t)((r >> 24) & 0xfffffff), (int32_t)((r >> 52) & 63) | ((int32_t)((r >> 58) & 1) << 8), 0});
  } else {
    const RecQuad& f = pt.rm[mt].first[slot - n0s];
    if (f.wid >= 0) {
      const int cnt1 = 1 + (int)((uint32_t)f.flags >> 9);
      for (int q = 0; q < cnt1; q++) { RecQuad r = q == 0 ? f : pt.rm[mt].extra[f.link + q - 1]; r.flags &= 0x1ff; r.link = 0; out.push_back(r); }
    }
  }
}

int gaml_hip_debug_fold_check(gaml_hip_ctx* c, int rs, int64_t* out6) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out6) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  for (int mt = 0; mt < 2; mt++) for (const Window& w : s.mate[mt].wins) if (w.first < 0 && w.count > 0) return fail(c, GAML_HIP_ESTATE, "host-only check: some windows' records exist in the device pool only (use gaml_hip_debug_tables_check)");
  PairTables with, without;
  build_pair_tables(s.mate[0], s.mate[1], with, true);
  build_pair_tables(s.mate[0], s.mate[1], without, false);
  int64_t checked = 0, bad = 0;
  const int64_t n = s.mate[0].n_local();
  std::vector<RecQuad> a, b;
  for (int mt = 0; mt < 2; mt++) {
    const ShortMate& m = s.mate[mt];
    // per (window, read, position): is it a record of an active single-node window?
    for (int64_t read = 0; read < n; read++) {
      a.clear(); b.clear();
      paired_base_records(with, with.slot_of_read[read], mt, a);
      paired_base_records(without, without.slot_of_read[read], mt, b);
      size_t ia = 0;
      for (size_t ib = 0; ib < b.size(); ib++) {
        checked++;
        const RecQuad& r = b[ib];
        if (ia < a.size() && a[ia].wid == r.wid && a[ia].pos == r.pos && a[ia].flags == r.flags) { ia++; continue; }
        // left out: must be a junction window whose first node's own window holds (read, position)
        const Window& j = m.wins[r.wid];
        bool ok = false;
        if (j.head >= 0) {
          auto it = m.solo_of_node.find(j.head);
          if (it != m.solo_of_node.end() && m.wins[it->second].active)
            for (size_t q = 0; q < b.size(); q++) ok = ok || (b[q].wid == it->second && b[q].pos == r.pos);
        }
        bad += !ok;
      }
      bad += ia != a.size();  // (a record with the rule that the tables without it do not hold)
    }
  }
  out6[0] = with.dropped_records[0]; out6[1] = with.dropped_records[1];
  out6[2] = with.class_count[0]; out6[3] = without.class_count[0];
  out6[4] = checked; out6[5] = bad;
  return bad ? fail(c, GAML_HIP_ESTATE, "record tables: a record was left out that is not always overwritten") : GAML_HIP_OK;
}

// The library's own radix sort and running maximum (radix_sort.hip.h) on caller data, for the tests: keys[n] (+ payload
// vals[n], null: keys only) sorted stably on bits [begin_bit, end_bit) in place; run_max (null: skip) receives the
// inclusive running maximum of the SORTED payload (or of the sorted keys when there is no payload).
int gaml_hip_debug_radix_sort(gaml_hip_ctx* c, uint64_t* keys, uint64_t* vals, int64_t n, int begin_bit, int end_bit, uint64_t* run_max) {
  MULTI_SHARD0(c);
  if (!c || c->device < 0 || !keys || n < 0 || begin_bit < 0 || end_bit > 64) return fail(c, c ? GAML_HIP_EINVAL : GAML_HIP_EINVAL, "bad arguments");
  if (n == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  typedef rs_u64 u64;
  DevBuf k_in, k_out, k_tmp, v_in, v_out, v_tmp, hist, rm, mx;
  const size_t bytes = (size_t)n * sizeof(u64);
  for (DevBuf* b : {&k_in, &k_out, &k_tmp, &mx}) HIP_TRY(c, b->reserve(bytes));
  if (vals) for (DevBuf* b : {&v_in, &v_out, &v_tmp}) HIP_TRY(c, b->reserve(bytes));
  HIP_TRY(c, hist.reserve(rs_hist_bytes((size_t)n)));
  HIP_TRY(c, rm.reserve(rm_scratch_bytes((size_t)n)));
  hipStream_t st = c->stream;
  HIP_TRY(c, hipMemcpyAsync(k_in.p, keys, bytes, hipMemcpyHostToDevice, st));
  if (vals) HIP_TRY(c, hipMemcpyAsync(v_in.p, vals, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(c, rs_sort<u64>(k_in.as<u64>(), k_out.as<u64>(), k_tmp.as<u64>(), vals ? v_in.as<u64>() : (const u64*)nullptr, vals ? v_out.as<u64>() : (u64*)nullptr,
                          vals ? v_tmp.as<u64>() : (u64*)nullptr, (size_t)n, begin_bit, end_bit, hist.as<unsigned>(), st));
  if (run_max) HIP_TRY(c, rm_inclusive_max(vals ? v_out.as<u64>() : k_out.as<u64>(), mx.as<u64>(), (size_t)n, rm.as<u64>(), st));
  HIP_TRY(c, hipMemcpyAsync(keys, k_out.p, bytes, hipMemcpyDeviceToHost, st));
  if (vals) HIP_TRY(c, hipMemcpyAsync(vals, v_out.p, bytes, hipMemcpyDeviceToHost, st));
  if (run_max) HIP_TRY(c, hipMemcpyAsync(run_max, mx.p, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return 0;
}

// Host-only check of the static memo indices (PairTables::static_idx): tables of the windows that are active now,
// every compact-class pair looked at again from the window cache -- the two records' windows compared by their node
// walks, orientation rule and insert distance recomputed (graph.cc:1864-1876). out8 = {pairs with a static index, other
// compact-class pairs, violations (an index that differs, or a pair that qualifies and has none), then why the other
// pairs have none: a mate without record, records in different windows, orientation rule, distance outside the
// insert-size table, edit count / length code outside the memo}.
int gaml_hip_debug_static_check(gaml_hip_ctx* c, int rs, int64_t* out8) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out8) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  for (int mt = 0; mt < 2; mt++) for (const Window& w : s.mate[mt].wins) if (w.first < 0 && w.count > 0) return fail(c, GAML_HIP_ESTATE, "host-only check: some windows' records exist in the device pool only (use gaml_hip_debug_tables_check)");
  if (int e = paired_host_tabs(c, s)) return e;
  const int ins_n = (int)s.ins_tab.size();
  link_mate_windows(s.mate[0], s.mate[1]);
  PairTables pt;
  build_pair_tables(s.mate[0], s.mate[1], pt, true, ins_n);
  for (int k = 0; k < 8; k++) out8[k] = 0;
  const int64_t n0 = pt.class_count[0];
  out8[0] = pt.n0a; out8[1] = n0 - pt.n0a;
  const int codes = (int)std::min<size_t>(pt.len_combo.size(), kMemoCodes);
  for (int64_t slot = 0; slot < n0; slot++) {
    const uint64_t r1 = pt.rec8[0][slot], r2 = pt.rec8[1][slot];
    const int32_t read = pt.read_of_slot[slot];
    int why = 0;  // 0: qualifies
    int32_t idx = -1;
    if (r1 == kNoRec8 || r2 == kNoRec8) { idx = kStaticZero; }  // never scores: static, too
    else {
      const int32_t w1 = (int32_t)(r1 & 0xffffff), w2 = (int32_t)(r2 & 0xffffff);
      if (*s.mate[0].win_walk[w1] != *s.mate[1].win_walk[w2]) why = 4;
      else {
        const int32_t p1 = (int32_t)((r1 >> 24) & 0xfffffff), p2 = (int32_t)((r2 >> 24) & 0xfffffff);
        const int32_t e1 = (int32_t)((r1 >> 52) & 63), e2 = (int32_t)((r2 >> 52) & 63), o1 = (int32_t)((r1 >> 58) & 1), o2 = (int32_t)((r2 >> 58) & 1);
        const int32_t L1 = s.mate[0].lens[read], L2 = s.mate[1].lens[read];
        int32_t dist = -1;
        if (o1 != o2) {  // graph.cc:1864-1876 on window positions (both alignments get the window's shift)
          if (p1 < p2) { if (o1 == 0 && o2 == 1) dist = p2 - p1 + L2; }
          else if (o1 == 1 && o2 == 0) dist = p1 - p2 + L1;
        }
        const int lc = pt.len_code[slot];
        if (dist < 0 && !(o1 != o2 && ((p1 < p2 && o1 == 0) || (p1 >= p2 && o1 == 1)))) why = 5;
        else if (dist < 0 || dist >= ins_n) why = 6;
        else if (e1 >= 7 || e2 >= 7 || lc >= codes) why = 7;
        else idx = ((lc * 7 + e1) * 7 + e2) * ins_n + dist;
      }
    }
    if (slot < pt.n0a) out8[2] += (why != 0 || idx != pt.static_idx[slot]);
    else { out8[2] += why == 0; if (why) out8[why]++; }
  }
  return out8[2] ? fail(c, GAML_HIP_ESTATE, "record tables: a static memo index is wrong or missing") : GAML_HIP_OK;
}

// per-block partial sums of the last blocking evaluation of paired read set rs (path set `set` of a batch launch; 0 for a
// single call), in block order [lane-per-pair classes | wave-per-pair blocks]: which
// block's sum differs when two routes that should agree bit for bit do not. Returns the number of blocks.
int32_t gaml_hip_debug_block_partials(gaml_hip_ctx* c, int rs, int32_t set, double* sums, int32_t* zeros, int32_t cap, int32_t* layout8) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1) return GAML_HIP_EINVAL;
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  if (!s.last_host_partials || set < 0 || set >= kMaxSets) return 0;
  const int n = s.last_blocks[set];
  const double* hs = (const double*)s.h_part_sum.p + (size_t)set * s.host_part_stride;
  const int* hz = (const int*)s.h_part_zero.p + (size_t)set * s.host_part_stride;
  for (int b = 0; b < n && b < cap; b++) { if (sums) sums[b] = hs[b]; if (zeros) zeros[b] = hz[b]; }
  if (layout8) {
    PairedArgs a; GridPlan gp;
    paired_base_args(c, s, a, gp);
    layout8[0] = gp.blocks0a; layout8[1] = gp.blocks0; layout8[2] = a.blocks01; layout8[3] = a.blocks012; layout8[4] = a.main_blocks; layout8[5] = a.total_blocks;
    layout8[6] = 0; layout8[7] = n;
  }
  return n;
}



// The device table build (table_build.hip.h) against the host restatement (host_model.cc build_pair_tables) on the windows
// that are active now: a fresh build into a scratch set of buffers, every array fetched and compared entry by entry. The
// host side works on a copy of the device pool (the records of windows the aligner's kernels filed exist nowhere else).
// out8 = {pairs, compact class, static part, <= 2 records, <= 4, more, entries compared, mismatches}.
int gaml_hip_debug_tables_check(gaml_hip_ctx* c, int rs, int64_t* out8) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out8) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  if (c->device < 0) return fail(c, GAML_HIP_ENODEVICE, "host-only context");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  HIP_TRY(c, hipSetDevice(c->device));
  if (s.rebuild.active) { if (int e = paired_build_continue(c, s, true)) return e; HIP_TRY(c, hipEventSynchronize(s.rebuild.done)); s.rebuild.active = false; s.rebuild.after.clear(); }
  if (int e = prepare_paired_tables(c, s)) return e;
  if (int e = pool_mirror(c, s, c->stream)) return e;
  if (int e = paired_upload_statics(c, s, c->stream)) return e;
  TableDev T;
  if (int e = paired_build_enqueue(c, s, T, c->stream)) return e;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int e = paired_build_collect(c, s, T)) return e;
  // host side
  ShortMate hm[2];
  for (int mt = 0; mt < 2; mt++) {
    const ShortMate& m = s.mate[mt];
    hm[mt].n_global = m.n_global; hm[mt].lo = m.lo; hm[mt].hi = m.hi; hm[mt].lens = m.lens;
    hm[mt].wins = m.wins;
    std::vector<int4> dp((size_t)s.dev[mt].pool_n);
    if (!dp.empty()) HIP_TRY(c, hipMemcpy(dp.data(), s.dev[mt].pool.p, dp.size() * sizeof(int4), hipMemcpyDeviceToHost));
    hm[mt].pool.resize(dp.size());
    for (size_t k = 0; k < dp.size(); k++) hm[mt].pool[k] = gaml_aligment{dp[k].y, dp[k].z & 0xff, dp[k].w, (dp[k].z >> 8) & 1};
    for (Window& w : hm[mt].wins) w.first = w.dfirst < 0 ? 0 : w.dfirst;
    for (Window& w : hm[mt].wins) if (w.dfirst < 0) { w.count = 0; }
  }
  PairTables pt;
  build_pair_tables(hm[0], hm[1], pt, KNOB(c, KEEP_DOMINATED) != 1, paired_static_ins_n(c, s));
  const int64_t n = s.mate[0].n_local();
  int64_t compared = 0, bad = 0;
  auto fetch = [&](const DevBuf& d, size_t bytes, std::vector<char>& out) -> int {
    out.resize(bytes);
    if (bytes) HIP_TRY(c, hipMemcpy(out.data(), d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
  };
  auto cmp = [&](const DevBuf& d, const void* host, size_t bytes, size_t elem, const char* what) -> int {
    std::vector<char> v;
    if (int e = fetch(d, bytes, v)) return e;
    int64_t b0 = bad;
    for (size_t k = 0; k < bytes / elem; k++) { compared++; if (memcmp(v.data() + k * elem, (const char*)host + k * elem, elem) != 0) bad++; }
    if (bad != b0 && getenv("GAML_HIP_TRACE_HOST")) fprintf(stderr, "tables_check: %s differs in %lld of %zu entries\n", what, (long long)(bad - b0), bytes / elem);
    return 0;
  };
  for (int k = 0; k < 4; k++) { compared++; bad += T.class_count[k] != pt.class_count[k]; }
  compared++; bad += T.n0a != pt.n0a;
  if (bad == 0) {
    const int64_t n0 = pt.class_count[0], n16 = n - n0;
    if (int e = cmp(T.slot_of_read, pt.slot_of_read.data(), (size_t)n * 4, 4, "slot_of_read")) return e;
    if (int e = cmp(T.read_of_slot, pt.read_of_slot.data(), (size_t)n * 4, 4, "read_of_slot")) return e;
    for (int mt = 0; mt < 2; mt++) {
      if (int e = cmp(T.rec8[mt], pt.rec8[mt].data(), (size_t)n0 * 8, 8, "rec8")) return e;
      if (int e = cmp(T.first[mt], pt.rm[mt].first.data(), (size_t)n16 * 16, 16, "first")) return e;
      if (int e = cmp(T.extra[mt], pt.rm[mt].extra.data(), pt.rm[mt].extra.size() * 16, 16, "extra")) return e;
      if (int e = cmp(T.inl[mt], pt.inl[mt].data(), pt.inl[mt].size() * 16, 16, "inl")) return e;
      compared++; bad += T.extras[mt] != (int64_t)pt.rm[mt].extra.size();
      compared++; bad += T.dropped[mt] != pt.dropped_records[mt];
    }
    if (int e = cmp(T.len_code, pt.len_code.data(), (size_t)n0, 1, "len_code")) return e;
    if (int e = cmp(T.static_idx, pt.static_idx.data(), (size_t)pt.n0a * 4, 4, "static_idx")) return e;
    if (int e = cmp(T.len12, pt.len12.data(), (size_t)n16 * 4, 4, "len12")) return e;
    compared++; bad += pt.len_combo != s.pt.len_combo;
  }
  out8[0] = n; out8[1] = T.class_count[0]; out8[2] = T.n0a; out8[3] = T.class_count[1]; out8[4] = T.class_count[2]; out8[5] = T.class_count[3];
  out8[6] = compared; out8[7] = bad;
  return bad ? fail(c, GAML_HIP_ESTATE, "record tables: the device build differs from the host restatement") : GAML_HIP_OK;
}

int gaml_hip_debug_occ_route(gaml_hip_ctx* c, int rs, int64_t* out6) {
  MULTI_SHARD0(c);
  if (!c || !out6 || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const PairedSet::OccDev& D = c->paireds[c->handles[rs].idx]->occdev;
  out6[0] = D.dev_calls; out6[1] = D.host_calls; out6[2] = D.fallbacks; out6[3] = D.compactions;
  out6[4] = (int64_t)(D.pool_used[0] + D.pool_used[1]); out6[5] = (int64_t)D.shared.size();
  return GAML_HIP_OK;
}

int gaml_hip_debug_aligner_routes(gaml_hip_ctx* c, int64_t* out4) {
  MULTI_SHARD0(c);
  if (!c || !out4) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  for (int k = 0; k < 4; k++) out4[k] = c->aln_routes[k];
  return GAML_HIP_OK;
}

// the resident read-major table of a single-end set against build_read_major, entry by entry; changes no state
int gaml_hip_debug_single_table_check(gaml_hip_ctx* c, int rs, int64_t* out4) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 0 || !out4) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const SingleSet& s = *c->singles[c->handles[rs].idx];
  ReadMajor want;
  build_read_major(s.mate, nullptr, want);
  out4[0] = (int64_t)(want.first.size() + want.extra.size()); out4[1] = out4[2] = out4[3] = 0;
  if (c->device < 0) return GAML_HIP_OK;
  const bool by_device = s.td.built_generation == s.mate.active_generation;
  if (!by_device && s.dev.uploaded_generation != s.mate.active_generation) return fail(c, GAML_HIP_ESTATE, "the resident table is older than the window cache: score a path set first");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int64_t extras = (int64_t)s.rm.extra.size();
  if (by_device) {
    int heads = 0;
    if (s.td.built_records > 0) HIP_TRY(c, hipMemcpy(&heads, s.td.zero.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost));
    extras = s.td.built_records - heads;
  }
  if (extras != (int64_t)want.extra.size()) out4[3]++;
  if (s.dev.first.cap < want.first.size() * sizeof(RecQuad) || (extras > 0 && s.dev.extra.cap < (size_t)extras * sizeof(RecQuad))) { out4[3]++; return GAML_HIP_OK; }
  std::vector<RecQuad> first(want.first.size()), extra((size_t)std::max<int64_t>(0, extras));
  if (!first.empty()) HIP_TRY(c, hipMemcpy(first.data(), s.dev.first.p, first.size() * sizeof(RecQuad), hipMemcpyDeviceToHost));
  if (!extra.empty()) HIP_TRY(c, hipMemcpy(extra.data(), s.dev.extra.p, extra.size() * sizeof(RecQuad), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < first.size(); i++) out4[1] += memcmp(&first[i], &want.first[i], sizeof(RecQuad)) != 0;
  for (size_t i = 0; i < std::min(extra.size(), want.extra.size()); i++) out4[2] += memcmp(&extra[i], &want.extra[i], sizeof(RecQuad)) != 0;
  return GAML_HIP_OK;
}

int gaml_hip_debug_occ_check(gaml_hip_ctx* c, int rs, int64_t* out4) {
  MULTI_SHARD0(c);
  if (!c || !out4 || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  PairedSet& ps = *c->paireds[c->handles[rs].idx];
  const PairedSet::OccDev& D = ps.occdev;
  out4[0] = out4[1] = out4[2] = out4[3] = 0;
  if (!D.image_stale) return GAML_HIP_OK;  // the last call did not take the device route (or the images were rebuilt since)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const PlanView& v = ps.planner.view();
  for (int mt = 0; mt < 2; mt++) {
    OccImage im;  // what the host route would have written for this set
    im.build(ps.mate[mt].wins.size(), v, mt);
    const size_t n = im.occ12.size();
    std::vector<Occ12> dev(n);
    if (n) HIP_TRY(c, hipMemcpy(dev.data(), occdev_table(ps, mt), n * sizeof(Occ12), hipMemcpyDeviceToHost));
    for (size_t w = 0; w < n; w++) {
      const Occ12& h = im.occ12[w];
      const Occ12& d = dev[w];
      const bool absent = h.lo == ~0u && h.hi == ~0u;
      out4[0]++;
      if (!absent) out4[1]++;
      if (absent ? (d.lo != ~0u || d.hi != ~0u) : (d.lo != h.lo || d.hi != h.hi || d.rank != h.rank)) out4[2]++;
    }
    if (!im.general_wids.empty()) out4[3]++;
  }
  if (out4[2] || out4[3]) return fail(c, GAML_HIP_ESTATE, "device occurrence tables differ from the host image");
  return GAML_HIP_OK;
}

int32_t gaml_hip_debug_batch_bad_bases(gaml_hip_ctx* c, int rs, int64_t* out, int32_t cap) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || cap < 0 || (cap > 0 && !out)) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const std::vector<int64_t>& b = c->paireds[c->handles[rs].idx]->batch_bad;
  for (size_t k = 0; k < b.size() && k < (size_t)cap; k++) out[k] = b[k];
  return (int32_t)b.size();
}

int32_t gaml_hip_debug_pacbio_batch_bad_bases(gaml_hip_ctx* c, int rs, int64_t* out, int32_t cap) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 2 || cap < 0 || (cap > 0 && !out)) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const std::vector<int64_t>& b = c->pacbios[c->handles[rs].idx]->batch_bad;
  for (size_t k = 0; k < b.size() && k < (size_t)cap; k++) out[k] = b[k];
  return (int32_t)b.size();
}

// The LIVE record tables plus the live delta store (delta_dev.hip.h) against the host restatement, read by read. Looks and
// changes nothing: no rebuild started or finished, no tables prepared (gaml_hip_debug_tables_check does all three) -- it
// waits for the stream and copies back. The reference: build_pair_tables on a copy of the device pool over the windows the
// live tables and their lists took in (TableDev::held: the build's windows, then every window paired_delta_apply was
// given), which yields every read's records per mate in (window id, position) order without the always-overwritten
// junction records (KEEP_DOMINATED as the tables were built). While a rebuild runs beside the evaluations this covers the live
// tables and lists only. out12 = {pairs on the lists, of those from the compact class's static part / its other part /
// the <= 2-record class / <= 4 / more, pairs at the fixed stride with lists of up to 2 / of 3 to 4 records, long lists
// (spill area), entries compared, mismatches, records of later windows left out (the device's count)}.
int gaml_hip_debug_delta_check(gaml_hip_ctx* c, int rs, int64_t* out12) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out12) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  if (c->device < 0) return fail(c, GAML_HIP_ENODEVICE, "host-only context");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  for (int k = 0; k < 12; k++) out12[k] = 0;
  const TableDev& T = s.tab;
  if (!T.built || !s.delta_cap) return fail(c, GAML_HIP_ESTATE, "delta check: no live tables yet");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  static const bool trace = getenv("GAML_HIP_TRACE_HOST") != nullptr;
  int64_t compared = 0, bad = 0;
  int shown = 0;
  auto miss = [&](const char* what, int64_t read, int64_t x, int64_t y) {
    bad++;
    if (trace && shown++ < 16) fprintf(stderr, "delta_check: %s (read %lld: %lld, %lld)\n", what, (long long)read, (long long)x, (long long)y);
  };
  auto expect = [&](bool ok, const char* what, int64_t read, int64_t x, int64_t y) { compared++; if (!ok) miss(what, read, x, y); };
  // ---- the reference: the host restatement over the windows the live tables and lists hold
  ShortMate hm[2];
  int64_t left_out_ref = 0;
  for (int mt = 0; mt < 2; mt++) {
    const ShortMate& m = s.mate[mt];
    hm[mt].n_global = m.n_global; hm[mt].lo = m.lo; hm[mt].hi = m.hi; hm[mt].lens = m.lens;
    hm[mt].wins = m.wins;
    hm[mt].solo_of_node = m.solo_of_node;
    std::vector<int4> dp((size_t)s.dev[mt].pool_n);
    if (!dp.empty()) HIP_TRY(c, hipMemcpy(dp.data(), s.dev[mt].pool.p, dp.size() * sizeof(int4), hipMemcpyDeviceToHost));
    hm[mt].pool.resize(dp.size());
    for (size_t k = 0; k < dp.size(); k++) hm[mt].pool[k] = gaml_aligment{dp[k].y, dp[k].z & 0xff, dp[k].w, (dp[k].z >> 8) & 1};
    for (Window& w : hm[mt].wins) { w.active = false; w.first = w.dfirst < 0 ? 0 : w.dfirst; if (w.dfirst < 0) w.count = 0; }
    for (int32_t wid : T.held[mt]) hm[mt].wins[(size_t)wid].active = true;
  }
  const bool fold = !T.keep_dominated;
  if (fold) {
    std::vector<uint8_t> keep;
    for (int mt = 0; mt < 2; mt++)
      for (size_t k = T.held_built[mt]; k < T.held[mt].size(); k++) {
        const int32_t wid = T.held[mt][k];
        left_out_ref += hm[mt].wins[(size_t)wid].count - undominated_records(hm[mt], wid, keep);
      }
  }
  PairTables pt;
  build_pair_tables(hm[0], hm[1], pt, fold, 0);
  // ---- the device side
  const int64_t n = s.mate[0].n_local();
  const int64_t n0 = T.class_count[0], n01 = n0 + T.class_count[1], n_main = n01 + T.class_count[2], n16 = n - n0;
  int dst[kDsInts];
  HIP_TRY(c, hipMemcpy(dst, s.dstate.p, sizeof(dst), hipMemcpyDeviceToHost));
  const int* hst = (const int*)s.h_dstate.p;
  if (hst[kDsSeq] == s.dl_seq) { for (int k = 0; k < kDsInts; k++) expect(dst[k] == hst[k], "a device counter differs from its pinned copy", -1, dst[k], hst[k]); }
  else expect(false, "the pinned counters are not those of the last maintenance launch", -1, hst[kDsSeq], s.dl_seq);
  const int64_t nd = dst[kDsDirty], ns = dst[kDsSpill], top[2] = {dst[kDsTop0], dst[kDsTop1]};
  expect(nd >= 0 && nd <= (int64_t)s.delta_cap && ns >= 0 && ns <= (int64_t)s.cap_spill && top[0] >= 0 && top[0] <= (int64_t)s.cap_sprec && top[1] >= 0 && top[1] <= (int64_t)s.cap_sprec,
         "the store's counters exceed its capacity", -1, nd, ns);
  if (bad) { out12[9] = compared; out12[10] = bad; return fail(c, GAML_HIP_ESTATE, "delta lists: the store's counters are inconsistent"); }
  expect(dst[6] == left_out_ref, "records left out: the device's count differs from the reference's", -1, dst[6], left_out_ref);
  {
    const volatile int* h = hst;
    int64_t host_left = s.delta_left_out;
    if (h[kDsSeq] == s.dl_seq) host_left = s.delta_left_out_base + h[6];  // (what paired_refresh_counts would make of it)
    expect(host_left - s.delta_left_out_base == left_out_ref, "delta_records_left_out differs from the reference's", -1, host_left - s.delta_left_out_base, left_out_ref);
  }
  std::vector<int32_t> slot_of_read((size_t)n), dirty_of_slot((size_t)n), dl_slot((size_t)nd), dl_spill((size_t)nd), sp_slot((size_t)ns);
  std::vector<unsigned long long> rec8[2];
  std::vector<int4> first[2], extra[2], inl0, dl_rec[2], sp_rec[2];
  std::vector<int2> sp_rng[2];
  auto get = [&](const DevBuf& d, void* dstp, size_t bytes) -> int {
    if (bytes == 0) return 0;
    if (!d.p || d.cap < bytes) return fail(c, GAML_HIP_ESTATE, "delta check: a device buffer is smaller than the counters say");
    HIP_TRY(c, hipMemcpy(dstp, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
  };
  if (int e = get(T.slot_of_read, slot_of_read.data(), (size_t)n * 4)) return e;
  if (int e = get(T.dirty_of_slot, dirty_of_slot.data(), (size_t)n * 4)) return e;
  if (int e = get(s.dl_slot, dl_slot.data(), (size_t)nd * 4)) return e;
  if (int e = get(s.dl_spill, dl_spill.data(), (size_t)nd * 4)) return e;
  if (int e = get(s.sp_slot, sp_slot.data(), (size_t)ns * 4)) return e;
  inl0.resize((size_t)(2 * T.class_count[1] + 4 * T.class_count[2]));
  if (int e = get(T.inl[0], inl0.data(), inl0.size() * sizeof(int4))) return e;
  for (int mt = 0; mt < 2; mt++) {
    rec8[mt].resize((size_t)n0); first[mt].resize((size_t)n16); extra[mt].resize((size_t)T.extras[mt]);
    dl_rec[mt].resize((size_t)nd * 4); sp_rec[mt].resize((size_t)top[mt]); sp_rng[mt].resize((size_t)ns);
    if (int e = get(T.rec8[mt], rec8[mt].data(), (size_t)n0 * 8)) return e;
    if (int e = get(T.first[mt], first[mt].data(), (size_t)n16 * sizeof(int4))) return e;
    if (int e = get(T.extra[mt], extra[mt].data(), extra[mt].size() * sizeof(int4))) return e;
    if (int e = get(s.dl_rec[mt], dl_rec[mt].data(), dl_rec[mt].size() * sizeof(int4))) return e;
    if (int e = get(s.sp_rec[mt], sp_rec[mt].data(), sp_rec[mt].size() * sizeof(int4))) return e;
    if (int e = get(s.sp_rng[mt], sp_rng[mt].data(), (size_t)ns * sizeof(int2))) return e;
  }
  std::vector<int32_t> d_seen((size_t)nd, 0), sp_seen((size_t)ns, 0);
  std::vector<std::pair<int64_t, int64_t>> used[2];  // spill ranges in use
  int64_t on_lists = 0, long_lists = 0;
  std::vector<RecQuad> ref;
  auto same = [](const int4& v, const RecQuad& r) { return v.x == r.wid && v.y == r.pos && v.z == r.flags; };
  for (int64_t read = 0; read < n; read++) {
    const int32_t sl = slot_of_read[(size_t)read];
    if (sl < 0 || sl >= n) { expect(false, "slot_of_read out of range", read, sl, n); continue; }
    const int32_t d = dirty_of_slot[(size_t)sl];
    const int32_t l12 = (int32_t)((uint32_t)s.mate[0].lens[(size_t)read] | ((uint32_t)s.mate[1].lens[(size_t)read] << 16));
    if (d < 0) {  // a clean pair: the tables' own lists are complete
      for (int mt = 0; mt < 2; mt++) {
        ref.clear();
        paired_base_records(pt, pt.slot_of_read[(size_t)read], mt, ref);
        if (sl < n0) {
          const unsigned long long r = rec8[mt][(size_t)sl];
          if (r == kDirty8) { expect(false, "a pair carries the lists' mark without a delta index", read, sl, mt); continue; }
          const int4 v = make_int4((int)(r & 0xffffff), (int)((r >> 24) & 0xfffffff), (int)((r >> 52) & 63) | ((int)((r >> 58) & 1) << 8), 0);
          expect(r == kNoRec8 ? ref.empty() : (ref.size() == 1 && same(make_int4(v.x, v.y, v.z & 0x1ff, 0), ref[0])), "a clean compact pair's record differs (a later record missing from the lists?)", read, sl, (int64_t)ref.size());
        } else {
          const int4 f = first[mt][(size_t)(sl - n0)];
          if (f.x == kDirtyWid) { expect(false, "a pair carries the lists' mark without a delta index", read, sl, mt); continue; }
          const int64_t cnt = f.x < 0 ? 0 : 1 + (int64_t)((unsigned)f.z >> 9);
          expect(cnt == (int64_t)ref.size(), "a clean pair's list length differs (a later record missing from the lists?)", read, cnt, (int64_t)ref.size());
          if (cnt != (int64_t)ref.size()) continue;
          for (int64_t k = 0; k < cnt; k++) {
            int4 v = k == 0 ? f : (f.w + k - 1 < (int64_t)extra[mt].size() ? extra[mt][(size_t)(f.w + k - 1)] : make_int4(-9, 0, 0, 0));
            v.z &= 0x1ff;
            expect(same(v, ref[(size_t)k]), "a clean pair's record differs", read, k, mt);
          }
        }
      }
      continue;
    }
    // a pair on the delta lists
    on_lists++;
    if (d >= nd) { expect(false, "delta index beyond the store's count", read, d, nd); continue; }
    d_seen[(size_t)d]++;
    expect(dl_slot[(size_t)d] == sl, "dl_slot is not the pair's slot", read, dl_slot[(size_t)d], sl);
    out12[1 + (sl < T.n0a ? 0 : sl < n0 ? 1 : sl < n01 ? 2 : sl < n_main ? 3 : 4)]++;
    // the tables' mark, where the pair's class keeps it
    if (sl < n0) expect(rec8[0][(size_t)sl] == kDirty8, "compact pair without the lists' mark (rec8)", read, sl, 0);
    else {
      if (sl < n01) expect(inl0[(size_t)2 * (sl - n0)].x == kDirtyWid, "<= 2-record pair without the lists' mark (inline copy)", read, sl, 0);
      else if (sl < n_main) expect(inl0[(size_t)2 * (n01 - n0) + (size_t)4 * (sl - n01)].x == kDirtyWid, "<= 4-record pair without the lists' mark (inline copy)", read, sl, 0);
      expect(first[0][(size_t)(sl - n0)].x == kDirtyWid, "pair without the lists' mark (first)", read, sl, 0);
    }
    const int32_t sp = dl_spill[(size_t)d];
    const int4* st4[2] = {&dl_rec[0][(size_t)4 * d], &dl_rec[1][(size_t)4 * d]};
    size_t len[2];
    for (int mt = 0; mt < 2; mt++) { ref.clear(); paired_base_records(pt, pt.slot_of_read[(size_t)read], mt, ref); len[mt] = ref.size(); }
    if (sp < 0) {  // both lists at the fixed stride
      const int hw = st4[1][0].w;
      expect(st4[0][0].w == l12, "head word of mate 1 is not L1 | L2 << 16", read, st4[0][0].w, l12);
      expect(hw == (int)(len[0] | (len[1] << 8)), "head word of mate 2 does not hold the two list lengths", read, hw, (int64_t)(len[0] | (len[1] << 8)));
      expect(len[0] <= 4 && len[1] <= 4, "a list of more than 4 records at the fixed stride", read, (int64_t)len[0], (int64_t)len[1]);
      out12[std::max(len[0], len[1]) <= 2 ? 6 : 7]++;
      for (int mt = 0; mt < 2; mt++) {
        ref.clear();
        paired_base_records(pt, pt.slot_of_read[(size_t)read], mt, ref);
        for (int k = 0; k < 4; k++) {
          const int4 v = st4[mt][k];
          if (k < (int)ref.size()) expect(same(v, ref[(size_t)k]) && (k == 0 || v.w == 0), "a record at the fixed stride differs", read, k, mt);
          else expect(v.x == -1 && v.y == 0 && v.z == 0 && (k == 0 || v.w == 0), "an unused stride entry is not {-1, 0, 0, 0}", read, k, mt);
        }
      }
    } else {
      long_lists++;
      if (sp >= ns) { expect(false, "spill index beyond the store's count", read, sp, ns); continue; }
      sp_seen[(size_t)sp]++;
      expect(sp_slot[(size_t)sp] == sl, "sp_slot is not the pair's slot", read, sp_slot[(size_t)sp], sl);
      expect(len[0] > 4 || len[1] > 4, "a pair in the spill area whose lists fit the fixed stride", read, (int64_t)len[0], (int64_t)len[1]);
      for (int mt = 0; mt < 2; mt++) {
        ref.clear();
        paired_base_records(pt, pt.slot_of_read[(size_t)read], mt, ref);
        const int2 g = sp_rng[mt][(size_t)sp];
        expect(g.y == (int)ref.size(), "a spill range's length differs", read, g.y, (int64_t)ref.size());
        const bool in = g.x >= 0 && g.y >= 0 && (int64_t)g.x + g.y <= top[mt];
        expect(in, "a spill range reaches beyond the area's top", read, g.x, g.y);
        if (in && g.y > 0) used[mt].emplace_back(g.x, g.y);
        if (in && g.y == (int)ref.size())
          for (int k = 0; k < g.y; k++) { const int4 v = sp_rec[mt][(size_t)g.x + k]; expect(same(v, ref[(size_t)k]) && v.w == 0, "a record in the spill area differs", read, k, mt); }
        for (int k = 0; k < 4; k++) {  // the stride entries of a spilled pair: empty, the read lengths in the first spare word, no stale counts
          const int4 v = st4[mt][k];
          expect(v.x == -1 && v.y == 0 && v.z == 0 && v.w == (k == 0 && mt == 0 ? l12 : 0), "a spilled pair's stride entry is not empty (stale head word?)", read, k, mt);
        }
      }
    }
  }
  expect(on_lists == nd, "pairs with a delta index differ from the store's count", -1, on_lists, nd);
  for (int64_t d = 0; d < nd; d++) if (d_seen[(size_t)d] != 1) expect(false, "a delta index is used by no pair or by several", -1, d, d_seen[(size_t)d]);
  expect(long_lists == ns, "pairs with a spill index differ from the store's count", -1, long_lists, ns);
  for (int64_t q = 0; q < ns; q++) if (sp_seen[(size_t)q] != 1) expect(false, "a spill index is used by no pair or by several", -1, q, sp_seen[(size_t)q]);
  for (int mt = 0; mt < 2; mt++) {
    std::sort(used[mt].begin(), used[mt].end());
    for (size_t k = 1; k < used[mt].size(); k++) expect(used[mt][k - 1].first + used[mt][k - 1].second <= used[mt][k].first, "two spill ranges overlap", -1, used[mt][k - 1].first, used[mt][k].first);
  }
  out12[0] = on_lists; out12[8] = long_lists; out12[9] = compared; out12[10] = bad; out12[11] = dst[6];
  return bad ? fail(c, GAML_HIP_ESTATE, "delta lists: the live tables and lists differ from the host restatement") : GAML_HIP_OK;
}

// Which launches the delta maintenance chose so far (paired_delta_apply): out10 = {one-block launches of delta_apply_kernel
// <1>, <2>, <4>, <8>, multi-block launches, of those with the window list in device memory, windows cut across launches,
// records and windows of the last apply, the smallest <1> block used (0: none)}.
int gaml_hip_debug_delta_routes(gaml_hip_ctx* c, int rs, int64_t* out10) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || !out10) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  const PairedSet& s = *c->paireds[c->handles[rs].idx];
  for (int k = 0; k < 10; k++) out10[k] = s.dl_routes[k];
  return GAML_HIP_OK;
}

// The numbering of the live delta lists: for delta index d the READ of its pair and its spill index (-1: fixed stride).
// Returns the number of pairs on the lists; at most `cap` are written.
int32_t gaml_hip_debug_delta_numbering(gaml_hip_ctx* c, int rs, int32_t* reads, int32_t* spill, int32_t cap) {
  MULTI_SHARD0(c);
  if (!c || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 1 || cap < 0 || (cap > 0 && (!reads || !spill))) return fail(c, GAML_HIP_EINVAL, "bad arguments");
  if (c->device < 0) return fail(c, GAML_HIP_ENODEVICE, "host-only context");
  PairedSet& s = *c->paireds[c->handles[rs].idx];
  if (!s.tab.built || !s.delta_cap) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int dst[kDsInts];
  HIP_TRY(c, hipMemcpy(dst, s.dstate.p, sizeof(dst), hipMemcpyDeviceToHost));
  const int nd = dst[kDsDirty];
  if (nd < 0 || (size_t)nd > s.delta_cap) return fail(c, GAML_HIP_ESTATE, "delta lists: the store's count exceeds its capacity");
  const int k = std::min<int>(nd, cap);
  if (k == 0) return nd;
  const int64_t n = s.mate[0].n_local();
  std::vector<int32_t> slot((size_t)k), ros((size_t)n);
  HIP_TRY(c, hipMemcpy(slot.data(), s.dl_slot.p, (size_t)k * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(spill, s.dl_spill.p, (size_t)k * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(ros.data(), s.tab.read_of_slot.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (int d = 0; d < k; d++) reads[d] = slot[(size_t)d] >= 0 && slot[(size_t)d] < n ? ros[(size_t)slot[(size_t)d]] : -1;
  return nd;
}
