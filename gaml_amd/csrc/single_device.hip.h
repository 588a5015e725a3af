// single_device.hip.h -- single-end sets on the device route (gaml_hip_set_single_device, off by default): their pending
// windows aligned as one device batch, the host's record pool mirrored into device memory, the read-major table rebuilt by
// the kernels of single_tables.hip.h. The host window cache stays the authority: hits come back and are filed on the host
// (aln_file_hits), nothing is filed on the device, there are no delta lists.
// (one translation unit with gaml_hip.hip, which includes this file in front of single_launch.hip.h)
//
//   single_device_plain   the contexts the route serves: one device, no shards, no communicator
//   single_align_pending  the set's pending windows as ONE batch on the general route of the device aligner
//   single_sync_records   what launch_single and single_chunk_launch call where upload_mate stood: switch off, upload_mate;
//                         switch on, the mirror's suffix + a whole rebuild when the active windows changed
#pragma once

int gpu_align_pending(gaml_hip_ctx* c, ShortMate& m, AlignDev& d, AlignSmall* small, AlnJob* job_in, PairedSet* ps, int mt);  // aligner_launch.hip.h
bool aln_gpu_capable(const gaml_hip_ctx* c, const ShortMate& m);

// two-pass registration (prepare_single_host) wherever the switch is on and the context is a plain one; the device parts
// need a device on top of that
inline bool single_device_plain(const gaml_hip_ctx* c) { return c->single_device && !c->multi && !c->multi_shard && !c->comm && c->world == 1 && c->peers == 1; }
inline bool single_device_route(const gaml_hip_ctx* c) { return single_device_plain(c) && c->device >= 0; }

// The set's pending windows, one batch: the general route of the device aligner where the mate is capable (no PairedSet, no
// small-batch buffers: large batches' hits are ordered on the device, all are filed on the host), the host aligner where it
// is not -- gpu_align_pending decides, and the records are the same either way. The job's buffers live in the context.
int single_align_pending(gaml_hip_ctx* c, SingleSet& s) {
  ShortMate& m = s.mate;
  if (m.pending.empty()) return 0;
  AlnJob& job = c->single_job;
  job.prepared = false; job.enqueued = false; job.wstr.clear(); job.wins.clear(); job.blk.clear();
  const int64_t before = c->aln_windows;
  if (int e = gpu_align_pending(c, m, s.dev.aln, nullptr, &job, nullptr, 0)) return e;
  s.td.aligned_windows += c->aln_windows - before;  // (a batch the host aligner took leaves the context's count alone)
  return 0;
}

int single_sync_records(gaml_hip_ctx* c, SingleSet& s, hipStream_t st) {
  const ShortMate& m = s.mate;
  MateDev& d = s.dev;
  SingleTabDev& T = s.td;
  if (!single_device_route(c)) {
    const bool build = d.uploaded_generation != m.active_generation;
    if (int e = upload_mate(c, s.mate, s.rm, s.dev, st)) return e;
    if (build) { T.host_builds++; T.built_generation = ~0ull; }  // (the resident table is the host route's now)
    return 0;
  }
  if (d.pow_n == 0) {  // (as upload_mate does)
    d.pow_n = m.match_pow.size();
    HIP_TRY(c, d.pows.reserve(2 * d.pow_n * sizeof(double)));
    HIP_TRY(c, hipMemcpy(d.pows.p, m.mismatch_pow.data(), d.pow_n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.pows.as<double>() + d.pow_n, m.match_pow.data(), d.pow_n * sizeof(double), hipMemcpyHostToDevice));
  }
  // the mirror: the records filed since the last sync, 16 bytes each, through pinned staging on the evaluation's stream
  const size_t have = m.pool.size();
  if (have >= ((size_t)1 << 31)) return fail(c, GAML_HIP_ESTATE, "single-end set: the record pool outgrew the device route's 32-bit offsets");
  if (have * sizeof(gaml_aligment) > d.pool.cap) {  // grows geometrically; the old mirror goes, so everything travels again
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, d.pool.reserve(2 * have * sizeof(gaml_aligment)));
    d.pool_n = 0;
  }
  if ((size_t)d.pool_n < have) {
    const size_t bytes = (have - (size_t)d.pool_n) * sizeof(gaml_aligment);
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, bytes, &host);
    if (slot < 0) return slot;
    memcpy(host, m.pool.data() + d.pool_n, bytes);
    if (int e = stage_upload(c, s.stage, slot, d.pool.as<gaml_aligment>() + d.pool_n, bytes, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    T.mirrored += (int64_t)(have - (size_t)d.pool_n);
    d.pool_n = (int64_t)have;
  }
  if (T.built_generation == m.active_generation) return 0;
  // the window cache changed (or the host route built the resident table): rebuild the whole table
  const int64_t n = m.n_local();
  void* host = nullptr;
  const int slot = stage_acquire(c, s.stage, std::max<size_t>(1, m.wins.size()) * sizeof(StWin), &host);
  if (slot < 0) return slot;
  StWin* const hw = (StWin*)host;
  int n_hdr = 0;
  int64_t total = 0;
  for (size_t wid = 0; wid < m.wins.size(); wid++) {
    const Window& w = m.wins[wid];
    if (!w.active || w.count == 0 || w.pending) continue;
    hw[n_hdr++] = StWin{(int)w.first, w.count, (int)wid, (int)total};
    total += w.count;
  }
  if (total >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return fail(c, GAML_HIP_ESTATE, "single-end set: too many records for the device route's 32-bit indices");
  const size_t A = (size_t)total;
  const unsigned tiles = (unsigned)((A + kTbScanTile - 1) / kTbScanTile);
  // the table and the build's scratch (a build at a time per set, in stream order behind the one before); a buffer that has
  // to grow is given back first, so the stream is waited for: earlier evaluations may still read the old table
  const std::pair<DevBuf*, size_t> bufs[] = {
      {&d.first, std::max<size_t>(1, (size_t)n) * sizeof(RecQuad)}, {&d.extra, std::max<size_t>(1, A) * sizeof(RecQuad)},  // (records that are not heads: at most all of them)
      {&T.hdr, std::max<size_t>(1, (size_t)n_hdr) * sizeof(StWin)}, {&T.k_in, A * sizeof(rs_u64)}, {&T.k_out, A * sizeof(rs_u64)}, {&T.k_tmp, A * sizeof(rs_u64)},
      {&T.v_in, A * sizeof(unsigned)}, {&T.v_out, A * sizeof(unsigned)}, {&T.v_tmp, A * sizeof(unsigned)}, {&T.hist, rs_hist_bytes(A)},
      {&T.flag, A * sizeof(int)}, {&T.before, A * sizeof(int)}, {&T.tiles, (size_t)tiles * sizeof(int)}, {&T.zero, 16 * sizeof(int)}};
  bool grows = false;
  for (const auto& b : bufs) grows = grows || b.second > b.first->cap;
  if (grows) HIP_TRY(c, hipStreamSynchronize(st));
  for (const auto& b : bufs) HIP_TRY(c, b.first->reserve(b.second));
  if (A) { if (int e = stage_upload(c, s.stage, slot, T.hdr.p, (size_t)n_hdr * sizeof(StWin), st)) return e; }
  if (int e = stage_release(c, s.stage, slot, st)) return e;
  if (n) {
    hipLaunchKernelGGL(st_clear_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, d.first.as<int4>(), (int)n);
    HIP_TRY(c, hipGetLastError());
  }
  if (A) {
    int bits = 0;
    while (((int64_t)1 << bits) < n) bits++;  // ceil(log2(reads)): every read id fits
    const unsigned grid = (unsigned)std::min<size_t>((A + 255) / 256, 4096);
    int* const zero = T.zero.as<int>();
    HIP_TRY(c, hipMemsetAsync(zero, 0, 16 * sizeof(int), st));
    hipLaunchKernelGGL(st_keys_kernel, dim3(grid), dim3(256), 0, st, d.pool.as<int4>(), T.hdr.as<int4>(), n_hdr, (int)A, T.k_in.as<rs_u64>(), T.v_in.as<unsigned>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, rs_sort<unsigned>(T.k_in.as<rs_u64>(), T.k_out.as<rs_u64>(), T.k_tmp.as<rs_u64>(), T.v_in.as<unsigned>(), T.v_out.as<unsigned>(), T.v_tmp.as<unsigned>(), A, 0, bits,
                                 T.hist.as<unsigned>(), st));
    hipLaunchKernelGGL(st_heads_kernel, dim3(grid), dim3(256), 0, st, T.k_out.as<rs_u64>(), (int)A, T.flag.as<int>());
    // (tb_scan_*: exclusive prefix of A ints, "A - cnt[kTbClass0]" entries: `zero` stands in for the counters)
    hipLaunchKernelGGL(tb_scan_tiles_kernel, dim3(tiles), dim3(256), 0, st, T.flag.as<int>(), zero - kTbClass0, (int)A, T.tiles.as<int>());
    hipLaunchKernelGGL(tb_scan_top_kernel, dim3(1), dim3(1024), 0, st, T.tiles.as<int>(), (int)tiles, zero + 1);
    hipLaunchKernelGGL(tb_scan_apply_kernel, dim3(tiles), dim3(256), 0, st, T.flag.as<int>(), zero - kTbClass0, (int)A, T.tiles.as<int>(), T.before.as<int>());
    hipLaunchKernelGGL(st_fill_kernel, dim3(grid), dim3(256), 0, st, d.pool.as<int4>(), T.hdr.as<int4>(), n_hdr, T.k_out.as<rs_u64>(), T.v_out.as<unsigned>(), T.flag.as<int>(),
                       T.before.as<int>(), (int)A, (int)n, d.first.as<int4>(), d.extra.as<int4>());
    HIP_TRY(c, hipGetLastError());
  }
  T.built_generation = m.active_generation;
  T.built_records = total;
  T.builds++;
  d.uploaded_generation = ~0ull;  // (the host route must not trust its own generation once this table took over)
  s.rm.total_records = m.active_records;  // what feeds the algorithmic-byte statistic
  return 0;
}
