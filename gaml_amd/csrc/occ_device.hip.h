// occ_device.hip.h -- the occurrence tables of a whole-set call, built on the device (included by gaml_hip.hip only).
//
// A call whose paths are all new against the previous call's (the planner's whole-set case) used to rebuild the host
// images over every occurrence of the set (OccImage::build) and write them whole through the BAR. Every memo already
// holds its occurrences as table entries minus the path slot (PathMemo::pre): those stay in a device pool, and a call
// sends one descriptor {pool offset, slot} per path. occ_scatter_kernel then
//   * writes the entries into table (n & 1) of each mate, n = the call's device-route serial: {lo, hi | slot << 16, rank},
//     the bits OccImage::build writes, and appends the window ids to that table's list;
//   * clears the entries of the other table named in its list (the previous device-route call's set: its scoring launch
//     is done, in stream order) -- writing and clearing touch different buffers, the grid needs no barrier;
//   * marks windows that occur twice in the set (stamp per window = n): the host cannot see cheaply that two paths share
//     a window, the kernel can. The flag lands in pinned memory; the blocking call then discards its partials and
//     evaluates the set again on the host route (which builds the lists such windows need), and remembers the memo
//     combination so that it goes to the host route directly next time.
// The route is taken only where the result is bit-equal to the host route's: memos whose entries are all direct and name
// a window once, at most kOccMaxDesc paths, a blocking call on the resident route (thresholds written as before).
#pragma once

namespace {

constexpr int kOccMaxDesc = 32;  // paths per set on the device route (descriptors travel in the kernel arguments)

struct OccDesc { long long off; int slot, start; };  // pool offset of the path's entries, its slot, first occurrence index in the call
struct OccScatterArgs {
  const OccPre* pool[2];
  Occ12* dst[2];              // table written by this call
  int* dst_list[2];           // ... and its list of window ids
  Occ12* clr[2];              // the other table: entries named in its list are cleared
  const int* clr_list[2];
  unsigned* stamp[2];
  int* dup;                   // pinned host memory
  int n_desc, total[2], n_clr[2];
  unsigned serial;
  OccDesc desc[2][kOccMaxDesc];
};

__global__ void __launch_bounds__(kBlock) occ_scatter_kernel(const OccScatterArgs a) {
  const int t0 = a.total[0], t01 = t0 + a.total[1], c0 = t01 + a.n_clr[0], n = c0 + a.n_clr[1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < t01) {
      const int mt = i < t0 ? 0 : 1;
      const int j = mt ? i - t0 : i;
      int d = 0;
      while (d + 1 < a.n_desc && a.desc[mt][d + 1].start <= j) d++;
      const OccDesc& D = a.desc[mt][d];
      const OccPre e = a.pool[mt][D.off + (j - D.start)];
      Occ12* o = a.dst[mt] + e.wid;
      o->lo = e.lo; o->hi = e.hi | ((unsigned)D.slot << 16); o->rank = e.rank;
      a.dst_list[mt][j] = e.wid;
      if (atomicExch(a.stamp[mt] + e.wid, a.serial) == a.serial) *(volatile int*)a.dup = 1;
    } else {
      const int mt = i < c0 ? 0 : 1;
      const int j = mt ? i - c0 : i - t01;
      Occ12* o = a.clr[mt] + a.clr_list[mt][j];
      o->lo = ~0u; o->hi = ~0u; o->rank = -1;
    }
  }
}

// the scoring launch of this call goes to the resident copy of the tables (launch_paired)
bool paired_resident_route(const gaml_hip_ctx* c, const PairedSet& s) {
  return c->host_results && c->direct_write && KNOB(c, UPLOAD_ROUTE) == 0 && KNOB(c, NO_RESIDENT_TABLES) == 0;
}

// after pass 2's occurrence lists (planner.finish): may this call's tables be built on the device?
bool occdev_route_ok(const gaml_hip_ctx* c, PairedSet& s) {
  PairedSet::OccDev& D = s.occdev;
  if (!c->occ_route || KNOB(c, NO_OCC_DEVICE) != 0 || !paired_resident_route(c, s) || !s.persist.valid) return false;
  if (s.cfg.penalty_constant > 0) return false;  // (the scatter kernel knows nothing of the coverage layout: penalised whole-set calls keep the host route)
  if (s.planner.last_was_incremental()) return false;
  const std::vector<int32_t>& ids = s.planner.ids();
  if (ids.empty() || ids.size() > (size_t)kOccMaxDesc) return false;
  D.key.clear();
  for (int32_t id : ids) {
    const PathMemo& pm = s.planner.memo(id);
    if (!pm.pre_plain[0] || !pm.pre_plain[1]) return false;
    D.key.push_back((uint64_t)(uint32_t)id << 32 | pm.serial);
  }
  for (const auto& k : D.shared) if (k == D.key) return false;
  return true;
}

// the memo combination of this call shares windows between paths: the host route from now on
void occdev_note_shared(PairedSet::OccDev& D) {
  constexpr size_t kShared = 16;
  if (D.shared.size() < kShared) D.shared.push_back(D.key);
  else { D.shared[D.shared_next] = D.key; D.shared_next = (D.shared_next + 1) % kShared; }
}

// cold path: tables, lists and stamps for `n_windows` windows and `n_occ` occurrences per mate (all reset)
int occdev_reserve(gaml_hip_ctx* c, PairedSet& s, size_t n_windows, size_t n_occ, hipStream_t st) {
  PairedSet::OccDev& D = s.occdev;
  if (D.cap_w > 0 && n_windows <= D.cap_w && n_occ <= D.cap_list) return 0;  // (a set without windows still needs its tables)
  HIP_TRY(c, hipStreamSynchronize(st));
  D.cap_w = std::max(std::max<size_t>(4 * n_windows, (size_t)1 << 18), D.cap_w);
  D.cap_list = std::max(std::max<size_t>(2 * n_occ, (size_t)1 << 16), D.cap_list);
  for (int mt = 0; mt < 2; mt++) {
    for (int k = 0; k < 2; k++) {
      HIP_TRY(c, D.tab[mt][k].reserve(D.cap_w * sizeof(Occ12)));
      HIP_TRY(c, hipMemsetAsync(D.tab[mt][k].p, 0xff, D.cap_w * sizeof(Occ12), st));
      HIP_TRY(c, D.list[mt][k].reserve(D.cap_list * sizeof(int32_t)));
      D.list_n[mt][k] = 0;
    }
    HIP_TRY(c, D.stamp[mt].reserve(D.cap_w * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetAsync(D.stamp[mt].p, 0, D.cap_w * sizeof(uint32_t), st));
  }
  D.serial = 0;
  return 0;
}

// every memo of the set gets its range in the pool (new or rebuilt memos: uploaded, stream-ordered from pinned staging;
// the staging buffer's previous copies are done -- the blocking call that issued them saw its scoring launch end)
int occdev_upload(gaml_hip_ctx* c, PairedSet& s, hipStream_t st, size_t* bytes) {
  PairedSet::OccDev& D = s.occdev;
  const std::vector<int32_t>& ids = s.planner.ids();
  auto missing = [&](const PathMemo& pm, int mt) { return pm.dev_off[mt] < 0 || pm.dev_gen[mt] != D.pool_gen; };
  size_t need[2] = {0, 0}, whole[2] = {0, 0};
  for (int32_t id : ids)
    for (int mt = 0; mt < 2; mt++) { const PathMemo& pm = s.planner.memo(id); whole[mt] += pm.pre[mt].size(); if (missing(pm, mt)) need[mt] += pm.pre[mt].size(); }
  if (D.pool_used[0] + need[0] > D.pool_cap[0] || D.pool_used[1] + need[1] > D.pool_cap[1]) {
    // full: the ranges of memos outside this set become garbage -- start over with this set's (cold path)
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int mt = 0; mt < 2; mt++) {
      if (2 * whole[mt] > D.pool_cap[mt]) {
        D.pool_cap[mt] = std::max<size_t>(8 * whole[mt], 2 * D.pool_cap[mt]);
        HIP_TRY(c, D.pool[mt].reserve(D.pool_cap[mt] * sizeof(OccPre)));
      }
      D.pool_used[mt] = 0;
      need[mt] = whole[mt];
    }
    D.pool_gen++;
    D.compactions++;
  }
  *bytes = (need[0] + need[1]) * sizeof(OccPre);
  if (need[0] + need[1] == 0) return 0;
  HIP_TRY(c, D.stage.reserve(*bytes));
  OccPre* sp = (OccPre*)D.stage.p;
  for (int mt = 0; mt < 2; mt++) {
    const size_t at = D.pool_used[mt];
    size_t k = 0;
    for (int32_t id : ids) {
      PathMemo& pm = s.planner.memo(id);
      if (!missing(pm, mt)) continue;  // (also the second instance of a memo that occurs twice)
      pm.dev_off[mt] = (int64_t)(at + k);
      pm.dev_gen[mt] = D.pool_gen;
      if (!pm.pre[mt].empty()) memcpy(sp + k, pm.pre[mt].data(), pm.pre[mt].size() * sizeof(OccPre));
      k += pm.pre[mt].size();
    }
    if (k) HIP_TRY(c, hipMemcpyAsync(D.pool[mt].as<OccPre>() + at, sp, k * sizeof(OccPre), hipMemcpyHostToDevice, st));
    D.pool_used[mt] = at + k;
    sp += k;
  }
  return 0;
}

// the device route of this call: ranges resident, one scatter launch on `st` (ahead of the scoring launch)
int occdev_launch(gaml_hip_ctx* c, PairedSet& s, hipStream_t st, size_t* bytes) {
  PairedSet::OccDev& D = s.occdev;
  const std::vector<int32_t>& ids = s.planner.ids();
  if (D.pool_cap[0] == 0 || D.pool_cap[1] == 0) {
    // first use: room for many sets of this size (the 8 rotating sets of the headline at cfg3 hold ~8 x its occurrences)
    for (int mt = 0; mt < 2; mt++) {
      size_t all = 0;
      for (int32_t id : ids) all += s.planner.memo(id).pre[mt].size();
      D.pool_cap[mt] = std::max<size_t>(16 * all, (size_t)1 << 10);
      HIP_TRY(c, D.pool[mt].reserve(D.pool_cap[mt] * sizeof(OccPre)));
      D.pool_used[mt] = 0;
    }
    D.pool_gen++;
  }
  size_t n_occ[2] = {0, 0};
  for (int32_t id : ids) for (int mt = 0; mt < 2; mt++) n_occ[mt] += s.planner.memo(id).pre[mt].size();
  const size_t n_windows = std::max(s.mate[0].wins.size(), s.mate[1].wins.size());
  if (int e = occdev_reserve(c, s, n_windows, std::max(n_occ[0], n_occ[1]), st)) return e;
  if (int e = occdev_upload(c, s, st, bytes)) return e;
  HIP_TRY(c, D.dup.reserve(sizeof(int)));
  *(volatile int*)D.dup.p = 0;
  if (++D.serial == 0) {  // (2^32 calls) stamps from the previous round could read as this call's
    for (int mt = 0; mt < 2; mt++) HIP_TRY(c, hipMemsetAsync(D.stamp[mt].p, 0, D.cap_w * sizeof(uint32_t), st));
    D.serial = 1;
  }
  const int cur = (int)(D.serial & 1), other = cur ^ 1;
  OccScatterArgs a;
  memset(&a, 0, sizeof(a));
  a.n_desc = (int)ids.size();
  for (int mt = 0; mt < 2; mt++) {
    a.pool[mt] = D.pool[mt].as<OccPre>();
    a.dst[mt] = D.tab[mt][cur].as<Occ12>();
    a.dst_list[mt] = D.list[mt][cur].as<int>();
    a.clr[mt] = D.tab[mt][other].as<Occ12>();
    a.clr_list[mt] = D.list[mt][other].as<int>();
    a.stamp[mt] = D.stamp[mt].as<unsigned>();
    int start = 0;
    for (size_t k = 0; k < ids.size(); k++) {
      const PathMemo& pm = s.planner.memo(ids[k]);
      a.desc[mt][k] = OccDesc{(long long)pm.dev_off[mt], (int)k, start};  // slots are positions in a whole-set call
      start += (int)pm.pre[mt].size();
    }
    a.total[mt] = start;
    a.n_clr[mt] = D.list_n[mt][other];
    D.list_n[mt][cur] = start;
    D.list_n[mt][other] = 0;
  }
  a.dup = (int*)D.dup.dev;
  a.serial = D.serial;
  const int items = a.total[0] + a.total[1] + a.n_clr[0] + a.n_clr[1];
  if (items > 0) {
    hipLaunchKernelGGL(occ_scatter_kernel, dim3((unsigned)std::min(512, (items + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    HIP_TRY(c, hipGetLastError());
  }
  return 0;
}

// the table the scoring launch of a device-route call reads
const Occ12* occdev_table(const PairedSet& s, int mt) { return s.occdev.tab[mt][s.occdev.serial & 1].as<Occ12>(); }

// consumers of the host images (batches, debug dumps) after calls whose tables the device built
void paired_images_refresh(PairedSet& s) {
  if (!s.occdev.image_stale) return;
  s.planner.rebuild_images(s.mate, s.image);
  s.occdev.image_stale = false;
}

}  // namespace
