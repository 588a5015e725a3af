// advice.hip.h -- the advice move of a paired set (ExtendPathsAdv moves.cc:933-998) on the device.
// (included by gaml_hip.hip; one translation unit with it)
//
//   build  ReadSet::BuildAdviceIndex (graph.cc:323-342) on mate 2: the missing one-node windows of the long nodes are
//          registered in the window table the scorer uses and aligned as one batch (align_pending_pair); then
//            adv_keys_kernel     every record of those windows in the device pool -> key (pair << nb | node), payload its
//                                orientation; records the position filter drops (graph.cc:577 with max_pos = 0) get pair = N
//            rs_sort             stable by key: a pair's records of one window stay in window order -- (position, read) --
//                                so the first of each run of equal keys is the pair's first record in that window
//            adv_heads_kernel    run heads -> flag + per-pair count
//            adv_scan_*          exclusive prefix sums: per-pair offsets (CSR) and each head's place
//            adv_scatter_kernel  entry node << 1 | orientation at its place
//          The CSR stays resident; no record travels to the host.
//   query  rs1.GetPositions (graph.cc:651-712) + the candidate loop (moves.cc:964-973) on mate 1. The host registers the
//          missing windows of GetSubpathsFromPath(path) (small-batch alignment route) and sends one step per window
//          lookup of the walk {pool range, cur_pos}; then
//            adv_first_kernel    per pair the smallest key (step << 26 | record) over its records: its first slot
//            adv_last_kernel     per pair the largest key among its records AT THE FIRST SLOT'S ABSOLUTE POSITION: the
//                                record whose (edit, orientation) the slot ends up with
//            adv_mask_kernel     exclusion bits (path nodes and their twins) and reach bits over node ids
//            adv_count_kernel    per pair whose first slot ends with orientation 0: its GetAdviceIndex1 nodes that pass
//            adv_scan_*, adv_write_kernel   places and the list
//          Keys carry the call's serial in their top 16 bits (inverted for the minimum), so that the per-pair words need
//          no clearing per call. One read-back of the count (pinned), then one of the list.
#pragma once

namespace {

constexpr int kAdvBlock = 256;
constexpr int kAdvPer = 8;                          // items per thread of a scan tile
constexpr int kAdvTile = kAdvBlock * kAdvPer;
constexpr int kAdvStepBits = 22, kAdvRecBits = 26;  // query key: serial:16 | step:22 | record in window:26
constexpr unsigned long long kAdvStepMask = (1ull << kAdvStepBits) - 1, kAdvRecMask = (1ull << kAdvRecBits) - 1;

struct AdvWin { long long dfirst; int count; int node; };     // build: one long node's window
struct AdvStep { long long dfirst; int count; int cur_pos; };  // query: one window lookup of the walk

// ---- exclusive prefix sum of n ints into n long longs (+ the total at *total) ---------------------------------------------
// (Not the table build's tb_scan_*: its places are 32-bit and its total lands in that build's counter block; nor
// rs_scan_*, which scan digit histograms. The CSR offsets of the ABI are 64-bit.)
__device__ inline long long adv_block_exclusive(long long v, long long* sh, long long* block_total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kAdvBlock; d <<= 1) {
    const long long x = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const long long incl = sh[t];
  *block_total = sh[kAdvBlock - 1];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(kAdvBlock) void adv_scan_tiles_kernel(const int* __restrict__ in, long long n, long long* __restrict__ tile_sum) {
  __shared__ long long sh[kAdvBlock];
  const long long base = (long long)blockIdx.x * kAdvTile + (long long)threadIdx.x * kAdvPer;
  long long s = 0;
  for (int j = 0; j < kAdvPer; j++) if (base + j < n) s += in[base + j];
  long long tot;
  (void)adv_block_exclusive(s, sh, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}
// one block: the tile sums, in place, exclusive; the grand total to *total
__global__ __launch_bounds__(kAdvBlock) void adv_scan_top_kernel(long long* __restrict__ tile_sum, int n_tiles, long long* __restrict__ total) {
  __shared__ long long sh[kAdvBlock];
  long long carry = 0;
  for (int b = 0; b < n_tiles; b += kAdvBlock) {
    const int i = b + threadIdx.x;
    const long long v = i < n_tiles ? tile_sum[i] : 0;
    long long tot;
    const long long ex = adv_block_exclusive(v, sh, &tot);
    if (i < n_tiles) tile_sum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(kAdvBlock) void adv_scan_apply_kernel(const int* __restrict__ in, long long n, const long long* __restrict__ tile_sum,
                                                                  long long* __restrict__ out) {
  __shared__ long long sh[kAdvBlock];
  const long long base = (long long)blockIdx.x * kAdvTile + (long long)threadIdx.x * kAdvPer;
  int v[kAdvPer];
  long long s = 0;
  for (int j = 0; j < kAdvPer; j++) { v[j] = base + j < n ? in[base + j] : 0; s += v[j]; }
  long long tot;
  long long at = tile_sum[blockIdx.x] + adv_block_exclusive(s, sh, &tot);
  for (int j = 0; j < kAdvPer; j++) if (base + j < n) { out[base + j] = at; at += v[j]; }
}
// out[0 .. n) = exclusive prefix of in, the total to *total; tiles: ceil(n / kAdvTile) long longs of scratch
hipError_t adv_scan(const int* in, long long n, long long* out, long long* total, long long* tiles, hipStream_t st) {
  const int n_tiles = (int)((n + kAdvTile - 1) / kAdvTile);
  if (n_tiles == 0) return hipMemsetAsync(total, 0, sizeof(long long), st);
  hipLaunchKernelGGL(adv_scan_tiles_kernel, dim3((unsigned)n_tiles), dim3(kAdvBlock), 0, st, in, n, tiles);
  hipLaunchKernelGGL(adv_scan_top_kernel, dim3(1), dim3(kAdvBlock), 0, st, tiles, n_tiles, total);
  hipLaunchKernelGGL(adv_scan_apply_kernel, dim3((unsigned)n_tiles), dim3(kAdvBlock), 0, st, in, n, tiles, out);
  return hipGetLastError();
}

// ---- build ----------------------------------------------------------------------------------------------------------------
// one block per window (grid-stride); at[w]: where window w's keys start
__global__ __launch_bounds__(kAdvBlock) void adv_keys_kernel(const int4* __restrict__ pool, const AdvWin* __restrict__ wins, int n_wins,
                                                            const long long* __restrict__ at, int nb, unsigned long long n_pairs,
                                                            rs_u64* __restrict__ keys, unsigned* __restrict__ vals) {
  for (int w = blockIdx.x; w < n_wins; w += gridDim.x) {
    const AdvWin win = wins[w];
    const long long base = at[w];
    for (int k = threadIdx.x; k < win.count; k += kAdvBlock) {
      const int4 r = pool[win.dfirst + k];  // {window, position, edit | orient << 8, pair}
      const unsigned long long pair = r.y < kAdviceMinPos ? n_pairs : (unsigned long long)(unsigned)r.w;
      keys[base + k] = (pair << nb) | (unsigned long long)(unsigned)win.node;
      vals[base + k] = ((unsigned)r.z >> 8) & 1u;
    }
  }
}
__global__ __launch_bounds__(kAdvBlock) void adv_heads_kernel(const rs_u64* __restrict__ keys, long long n, int nb, unsigned long long n_pairs,
                                                             int* __restrict__ flag, int* __restrict__ cnt) {
  for (long long i = (long long)blockIdx.x * kAdvBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kAdvBlock) {
    const rs_u64 k = keys[i];
    const unsigned long long pair = k >> nb;
    const int head = pair < n_pairs && (i == 0 || keys[i - 1] != k);
    flag[i] = head;
    if (head) atomicAdd(&cnt[pair], 1);
  }
}
__global__ __launch_bounds__(kAdvBlock) void adv_scatter_kernel(const rs_u64* __restrict__ keys, const unsigned* __restrict__ vals, long long n, int nb,
                                                               const int* __restrict__ flag, const long long* __restrict__ place,
                                                               int* __restrict__ ent) {
  const unsigned long long node_mask = (1ull << nb) - 1;
  for (long long i = (long long)blockIdx.x * kAdvBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kAdvBlock)
    if (flag[i]) ent[place[i]] = (int)(((keys[i] & node_mask) << 1) | (vals[i] & 1u));
}

// ---- query ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAdvBlock) void adv_first_kernel(const int4* __restrict__ pool, const AdvStep* __restrict__ steps, int n_steps,
                                                             unsigned long long hi_min, unsigned long long* __restrict__ first) {
  for (int s = blockIdx.x; s < n_steps; s += gridDim.x) {
    const AdvStep st = steps[s];
    for (int k = threadIdx.x; k < st.count; k += kAdvBlock) {
      const int r = pool[st.dfirst + k].w;
      atomicMin(&first[r], hi_min | ((unsigned long long)s << kAdvRecBits) | (unsigned long long)k);
    }
  }
}
// the record a key names, and its absolute position on the path
__device__ inline int4 adv_record_of(const int4* pool, const AdvStep* steps, unsigned long long key, int* abs_pos) {
  const AdvStep st = steps[(key >> kAdvRecBits) & kAdvStepMask];
  const int4 r = pool[st.dfirst + (long long)(key & kAdvRecMask)];
  *abs_pos = st.cur_pos + r.y;
  return r;
}
__global__ __launch_bounds__(kAdvBlock) void adv_last_kernel(const int4* __restrict__ pool, const AdvStep* __restrict__ steps, int n_steps,
                                                            unsigned long long hi_max, const unsigned long long* __restrict__ first,
                                                            unsigned long long* __restrict__ last) {
  for (int s = blockIdx.x; s < n_steps; s += gridDim.x) {
    const AdvStep st = steps[s];
    for (int k = threadIdx.x; k < st.count; k += kAdvBlock) {
      const int4 r = pool[st.dfirst + k];
      int abs0;
      (void)adv_record_of(pool, steps, first[r.w], &abs0);  // (this call's key: the record itself took part in the minimum)
      if (st.cur_pos + r.y == abs0) atomicMax(&last[r.w], hi_max | ((unsigned long long)s << kAdvRecBits) | (unsigned long long)k);
    }
  }
}
// bits of the path's nodes and their twins (excl) and of the reach keys; both masks zeroed before
__global__ __launch_bounds__(kAdvBlock) void adv_mask_kernel(const int* __restrict__ path, int n_path, const int* __restrict__ reach, int n_reach,
                                                            unsigned* __restrict__ excl, unsigned* __restrict__ reach_bits) {
  for (int i = blockIdx.x * kAdvBlock + threadIdx.x; i < n_path + n_reach; i += gridDim.x * kAdvBlock) {
    if (i < n_path) {
      const int v = path[i];
      if (v >= 0) atomicOr(&excl[v >> 5], 3u << (v & 30));  // v and its twin v ^ 1 share a word
    } else {
      const int v = reach[i - n_path];
      atomicOr(&reach_bits[v >> 5], 1u << (v & 31));
    }
  }
}
__device__ inline bool adv_keep(int e, int flags, const unsigned* excl, const unsigned* reach_bits) {
  if (!(e & 1)) return false;  // not in GetAdviceIndex1
  const int v = e >> 1;
  if ((flags & GAML_HIP_ADVICE_ONLY_OUT) && ((excl[v >> 5] >> (v & 31)) & 1u)) return false;
  return (flags & GAML_HIP_ADVICE_ALLOW_GAPS) || ((reach_bits[v >> 5] >> (v & 31)) & 1u);
}
// a pair qualifies when it has a slot in this call and the record its first slot ends with has orientation 0 (moves.cc:965-966)
__global__ __launch_bounds__(kAdvBlock) void adv_count_kernel(const int4* __restrict__ pool, const AdvStep* __restrict__ steps, long long n_pairs,
                                                             unsigned long long hi_min, unsigned long long hi_max,
                                                             const unsigned long long* __restrict__ first, const unsigned long long* __restrict__ last,
                                                             const long long* __restrict__ offs, const int* __restrict__ ent, int flags,
                                                             const unsigned* __restrict__ excl, const unsigned* __restrict__ reach_bits,
                                                             int* __restrict__ cnt) {
  for (long long p = (long long)blockIdx.x * kAdvBlock + threadIdx.x; p < n_pairs; p += (long long)gridDim.x * kAdvBlock) {
    int c = 0;
    const unsigned long long f = first[p], l = last[p];
    if ((f >> 48) == (hi_min >> 48) && (l >> 48) == (hi_max >> 48)) {
      int abs_pos;
      const int4 r = adv_record_of(pool, steps, l, &abs_pos);
      if ((((unsigned)r.z >> 8) & 1u) == 0)
        for (long long q = offs[p]; q < offs[p + 1]; q++) c += adv_keep(ent[q], flags, excl, reach_bits);
    }
    cnt[p] = c;
  }
}
__global__ __launch_bounds__(kAdvBlock) void adv_write_kernel(long long n_pairs, const int* __restrict__ cnt, const long long* __restrict__ at,
                                                             const long long* __restrict__ offs, const int* __restrict__ ent, int flags,
                                                             const unsigned* __restrict__ excl, const unsigned* __restrict__ reach_bits,
                                                             int* __restrict__ out) {
  for (long long p = (long long)blockIdx.x * kAdvBlock + threadIdx.x; p < n_pairs; p += (long long)gridDim.x * kAdvBlock) {
    if (cnt[p] == 0) continue;
    long long o = at[p];
    for (long long q = offs[p]; q < offs[p + 1]; q++) {
      const int e = ent[q];
      if (adv_keep(e, flags, excl, reach_bits)) out[o++] = e >> 1;
    }
  }
}

unsigned adv_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + kAdvBlock - 1) / kAdvBlock, 4096)); }

// The development build checks every device index and candidate list against the host restatement (host_model.cc).
#ifdef GAML_HIP_DEV
#define DEV_CHECKS true
#else
#define DEV_CHECKS false
#endif

// ---- host side ------------------------------------------------------------------------------------------------------------
int advice_set(gaml_hip_ctx* c, int rs, PairedSet** out) {
  if (!c || rs < 0 || rs >= (int)c->handles.size()) return fail(c, GAML_HIP_EINVAL, "advice: no such read set");
  if (c->handles[rs].kind != 1) return fail(c, GAML_HIP_EINVAL, "advice: not a paired read set");
  if (c->peers > 1 && !c->multi_shard)
    return fail(c, GAML_HIP_ESTATE, "advice: not served on rank-per-process contexts (gaml_hip_create_multi serves several devices)");
  if (c->pending_open) return fail(c, GAML_HIP_ESTATE, "advice: an evaluation is open (gaml_hip_eval_begin without _finish)");
  if (!c->have_graph) return fail(c, GAML_HIP_ESTATE, "advice: no graph");
  *out = c->paireds[c->handles[rs].idx].get();
  return 0;
}

// records for the windows registered since the last alignment; on a device every record then sits in the device pool
int advice_align(gaml_hip_ctx* c, PairedSet& ps) {
  if (int e = align_pending_pair(c, ps)) return e;
  if (c->device >= 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (int e = pool_mirror(c, ps, c->stream)) return e;
  }
  return 0;
}

int advice_build_dev(gaml_hip_ctx* c, PairedSet& ps, const std::vector<int32_t>& wids) {
  AdviceDev& A = ps.adv;
  const ShortMate& m = ps.mate[1];
  const hipStream_t st = c->stream;
  const long long N = m.n_local();
  std::vector<AdvWin> wins;
  std::vector<long long> at;
  long long R = 0;
  for (int32_t wid : wids) {
    const Window& w = m.wins[wid];
    if (w.count == 0) continue;
    if (w.dfirst < 0) return fail(c, GAML_HIP_ESTATE, "advice: a window's records are not in the device pool");
    wins.push_back(AdvWin{(long long)w.dfirst, w.count, (*m.win_walk[wid])[0]});
    at.push_back(R);
    R += w.count;
  }
  const int nb = bits_for((uint64_t)std::max<int32_t>(1, c->g.n() - 1));
  const int end_bit = nb + bits_for((uint64_t)N);
  if (end_bit > 64 || R >= ((long long)1 << 31)) return fail(c, GAML_HIP_EINVAL, "advice: index too large");
  const size_t tiles_r = (size_t)(R + kAdvTile - 1) / kAdvTile, tiles_p = (size_t)(N + kAdvTile - 1) / kAdvTile;
  // scratch: keys x3 | payloads x3 | flags | places | scan tiles + one total | windows | their starts | sort histogram
  const size_t o_vals = (size_t)R * 3 * sizeof(rs_u64), o_flag = o_vals + align16((size_t)R * 3 * sizeof(unsigned));
  const size_t o_place = o_flag + align16((size_t)R * sizeof(int)), o_tiles = o_place + (size_t)R * sizeof(long long);
  const size_t o_wins = o_tiles + (std::max(tiles_r, tiles_p) + 2) * sizeof(long long), o_at = o_wins + wins.size() * sizeof(AdvWin);
  const size_t o_hist = align16(o_at + at.size() * sizeof(long long)), bytes = o_hist + rs_hist_bytes((size_t)R);
  HIP_TRY(c, A.scratch.reserve(bytes));
  char* S = A.scratch.as<char>();
  rs_u64* keys = (rs_u64*)S;
  unsigned* vals = (unsigned*)(S + o_vals);
  int* flag = (int*)(S + o_flag);
  long long* place = (long long*)(S + o_place);
  long long* tiles = (long long*)(S + o_tiles);
  long long* spare_total = tiles + std::max(tiles_r, tiles_p) + 1;
  HIP_TRY(c, A.offs.reserve((size_t)(N + 1) * sizeof(long long)));
  HIP_TRY(c, A.cnt.reserve((size_t)std::max<long long>(1, N) * sizeof(int)));
  const size_t in_bytes = wins.size() * sizeof(AdvWin) + at.size() * sizeof(long long);
  HIP_TRY(c, A.h_in.reserve(in_bytes + 16));
  memcpy(A.h_in.p, wins.data(), wins.size() * sizeof(AdvWin));
  memcpy((char*)A.h_in.p + wins.size() * sizeof(AdvWin), at.data(), at.size() * sizeof(long long));
  if (in_bytes) HIP_TRY(c, hipMemcpyAsync(S + o_wins, A.h_in.p, in_bytes, hipMemcpyHostToDevice, st));
  if (N > 0) HIP_TRY(c, hipMemsetAsync(A.cnt.p, 0, (size_t)N * sizeof(int), st));
  if (R > 0) {
    hipLaunchKernelGGL(adv_keys_kernel, dim3((unsigned)std::min<size_t>(wins.size(), 4096)), dim3(kAdvBlock), 0, st, ps.dev[1].pool.as<int4>(),
                       (const AdvWin*)(S + o_wins), (int)wins.size(), (const long long*)(S + o_at), nb, (unsigned long long)N, keys, vals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, rs_sort<unsigned>(keys, keys + R, keys + 2 * R, vals, vals + R, vals + 2 * R, (size_t)R, 0, end_bit, (unsigned*)(S + o_hist), st));
    hipLaunchKernelGGL(adv_heads_kernel, dim3(adv_grid(R)), dim3(kAdvBlock), 0, st, keys + R, R, nb, (unsigned long long)N, flag, A.cnt.as<int>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, adv_scan(flag, R, place, spare_total, tiles, st));
  }
  HIP_TRY(c, adv_scan(A.cnt.as<int>(), N, A.offs.as<long long>(), A.offs.as<long long>() + N, tiles, st));
  HIP_TRY(c, hipMemcpyAsync(A.h_in.p, A.offs.as<long long>() + N, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  long long n_ent = 0;
  memcpy(&n_ent, A.h_in.p, sizeof(long long));
  if (n_ent < 0 || n_ent > R) return fail(c, GAML_HIP_ESTATE, "advice: index size out of range");
  HIP_TRY(c, A.ent.reserve((size_t)std::max<long long>(1, n_ent) * sizeof(int)));
  HIP_TRY(c, A.out.reserve((size_t)std::max<long long>(1, n_ent) * sizeof(int)));  // a candidate list never outgrows the index
  if (R > 0) {
    hipLaunchKernelGGL(adv_scatter_kernel, dim3(adv_grid(R)), dim3(kAdvBlock), 0, st, keys + R, vals + R, R, nb, flag, place, A.ent.as<int>());
    HIP_TRY(c, hipGetLastError());
  }
  // per-pair query state: keys stamped with the call's serial, reset only when the serial wraps
  const size_t np = (size_t)std::max<long long>(1, N);
  HIP_TRY(c, A.first.reserve(np * sizeof(unsigned long long)));
  HIP_TRY(c, A.last.reserve(np * sizeof(unsigned long long)));
  HIP_TRY(c, A.at.reserve((size_t)(N + 1) * sizeof(long long)));
  HIP_TRY(c, A.tiles.reserve((tiles_p + 1) * sizeof(long long)));
  HIP_TRY(c, hipMemsetAsync(A.first.p, 0xff, np * sizeof(unsigned long long), st));
  HIP_TRY(c, hipMemsetAsync(A.last.p, 0, np * sizeof(unsigned long long), st));
  const size_t words = ((size_t)c->g.n() + 31) / 32;
  HIP_TRY(c, A.mask.reserve(std::max<size_t>(1, 2 * words) * sizeof(unsigned)));
  HIP_TRY(c, hipStreamSynchronize(st));
  A.n_ent = n_ent;
  A.serial = 0;
  return 0;
}

// the device index equals the host restatement's (A.h_offs / A.h_ent)
bool advice_index_matches(gaml_hip_ctx* c, PairedSet& ps) {
  const AdviceDev& A = ps.adv;
  std::vector<int64_t> offs(A.h_offs.size());
  std::vector<int32_t> ent((size_t)A.n_ent);
  if (hipMemcpy(offs.data(), A.offs.p, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (A.n_ent && hipMemcpy(ent.data(), A.ent.p, ent.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
  return offs == A.h_offs && ent == A.h_ent;
}

int advice_query_dev(gaml_hip_ctx* c, PairedSet& ps, const std::vector<AdviceStep>& steps, const int32_t* path, int32_t n,
                     const int32_t* reach, int32_t n_reach, int32_t flags, std::vector<int32_t>& list) {
  AdviceDev& A = ps.adv;
  const ShortMate& m = ps.mate[0];
  const hipStream_t st = c->stream;
  const long long N = m.n_local();
  list.clear();
  if (N == 0) return 0;
  if (steps.size() > kAdvStepMask) return fail(c, GAML_HIP_EINVAL, "advice: path too long");
  if (++A.serial >= 0xffffu) {
    HIP_TRY(c, hipMemsetAsync(A.first.p, 0xff, (size_t)N * sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemsetAsync(A.last.p, 0, (size_t)N * sizeof(unsigned long long), st));
    A.serial = 1;
  }
  const unsigned long long hi_min = (unsigned long long)(0xffffu - A.serial) << 48, hi_max = (unsigned long long)A.serial << 48;
  // one input block: steps | path | reach
  const size_t o_path = steps.size() * sizeof(AdvStep), o_reach = o_path + (size_t)n * sizeof(int32_t);
  const size_t bytes = o_reach + (size_t)n_reach * sizeof(int32_t);
  HIP_TRY(c, A.h_in.reserve(bytes + 16));
  HIP_TRY(c, A.in.reserve(bytes + 16));
  AdvStep* hs = (AdvStep*)A.h_in.p;
  for (size_t i = 0; i < steps.size(); i++) {
    const Window& w = m.wins[steps[i].wid];
    if (w.dfirst < 0) return fail(c, GAML_HIP_ESTATE, "advice: a window's records are not in the device pool");
    if ((unsigned long long)w.count > kAdvRecMask + 1) return fail(c, GAML_HIP_EINVAL, "advice: window too large");
    hs[i] = AdvStep{(long long)w.dfirst, w.count, steps[i].cur_pos};
  }
  if (n) memcpy((char*)A.h_in.p + o_path, path, (size_t)n * sizeof(int32_t));
  if (n_reach) memcpy((char*)A.h_in.p + o_reach, reach, (size_t)n_reach * sizeof(int32_t));
  if (bytes) HIP_TRY(c, hipMemcpyAsync(A.in.p, A.h_in.p, bytes, hipMemcpyHostToDevice, st));
  const AdvStep* d_steps = A.in.as<AdvStep>();
  const int4* pool = ps.dev[0].pool.as<int4>();
  const int n_steps = (int)steps.size();
  const size_t words = ((size_t)c->g.n() + 31) / 32;
  unsigned* excl = A.mask.as<unsigned>();
  unsigned* reach_bits = excl + words;
  HIP_TRY(c, hipMemsetAsync(excl, 0, std::max<size_t>(1, 2 * words) * sizeof(unsigned), st));
  if (n + n_reach > 0)
    hipLaunchKernelGGL(adv_mask_kernel, dim3(adv_grid(n + n_reach)), dim3(kAdvBlock), 0, st, (const int*)((const char*)A.in.p + o_path), n,
                       (const int*)((const char*)A.in.p + o_reach), n_reach, excl, reach_bits);
  if (n_steps > 0) {
    const unsigned g = (unsigned)std::min(n_steps, 4096);
    hipLaunchKernelGGL(adv_first_kernel, dim3(g), dim3(kAdvBlock), 0, st, pool, d_steps, n_steps, hi_min, A.first.as<unsigned long long>());
    hipLaunchKernelGGL(adv_last_kernel, dim3(g), dim3(kAdvBlock), 0, st, pool, d_steps, n_steps, hi_max, A.first.as<unsigned long long>(),
                       A.last.as<unsigned long long>());
  }
  hipLaunchKernelGGL(adv_count_kernel, dim3(adv_grid(N)), dim3(kAdvBlock), 0, st, pool, d_steps, N, hi_min, hi_max, A.first.as<unsigned long long>(),
                     A.last.as<unsigned long long>(), A.offs.as<long long>(), A.ent.as<int>(), flags, excl, reach_bits, A.cnt.as<int>());
  HIP_TRY(c, hipGetLastError());
  long long* at = A.at.as<long long>();
  HIP_TRY(c, adv_scan(A.cnt.as<int>(), N, at, at + N, A.tiles.as<long long>(), st));
  hipLaunchKernelGGL(adv_write_kernel, dim3(adv_grid(N)), dim3(kAdvBlock), 0, st, N, A.cnt.as<int>(), at, A.offs.as<long long>(), A.ent.as<int>(),
                     flags, excl, reach_bits, A.out.as<int>());
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, A.h_out.reserve(sizeof(long long)));
  HIP_TRY(c, hipMemcpyAsync(A.h_out.p, at + N, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  long long count = 0;
  memcpy(&count, A.h_out.p, sizeof(long long));
  if (count < 0 || count > A.n_ent) return fail(c, GAML_HIP_ESTATE, "advice: candidate count out of range");
  if (count > 0) {
    HIP_TRY(c, A.h_out.reserve((size_t)count * sizeof(int32_t)));
    HIP_TRY(c, hipMemcpyAsync(A.h_out.p, A.out.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    list.assign((const int32_t*)A.h_out.p, (const int32_t*)A.h_out.p + count);
  }
  return 0;
}

// the records of windows (wid, tag) as spans for the host restatement: the host pool on host-only contexts; on a device
// copied back from the device pool (development build: the device's answers are checked against the restatement)
int advice_spans(gaml_hip_ctx* c, PairedSet& ps, int mt, const std::vector<int32_t>& wids, const std::vector<int32_t>& at,
                 std::vector<gaml_aligment>& buf, std::vector<AdviceSpan>& spans) {
  const ShortMate& m = ps.mate[mt];
  if (c->device < 0) { advice_host_spans(m, wids, at, spans); return 0; }
  int64_t total = 0;
  for (int32_t wid : wids) total += m.wins[wid].count;
  std::vector<int4> tmp((size_t)total);
  buf.resize((size_t)total);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int64_t o = 0;
  for (int32_t wid : wids) {
    const Window& w = m.wins[wid];
    if (w.count) HIP_TRY(c, hipMemcpy(tmp.data() + o, ps.dev[mt].pool.as<int4>() + w.dfirst, (size_t)w.count * sizeof(int4), hipMemcpyDeviceToHost));
    o += w.count;
  }
  for (int64_t i = 0; i < total; i++) buf[(size_t)i] = gaml_aligment{tmp[i].y, tmp[i].z & 0xff, tmp[i].w, (tmp[i].z >> 8) & 1};
  spans.clear();
  o = 0;
  for (size_t k = 0; k < wids.size(); k++) {
    const int32_t cnt = m.wins[wids[k]].count;
    spans.push_back(AdviceSpan{buf.data() + o, cnt, at[k]});
    o += cnt;
  }
  return 0;
}

}  // namespace

// ---- this context's pairs (what the C ABI below and multi.hip call) ---------------------------------------------------------
namespace gaml {
int ctx_advice_build(gaml_hip_ctx* c, int rs, int32_t threshold) {
  PairedSet* ps = nullptr;
  if (int e = advice_set(c, rs, &ps)) return e;
  AdviceDev& A = ps->adv;
  if (A.built) return GAML_HIP_OK;  // graph.cc:324: the first threshold stays
  std::vector<int32_t> wids, nodes;
  advice_register_index(c->g, ps->mate[1], threshold, wids);
  if (int e = advice_align(c, *ps)) return e;
  for (int32_t wid : wids) nodes.push_back((*ps->mate[1].win_walk[wid])[0]);
  if (c->device >= 0) {
    if (int e = advice_build_dev(c, *ps, wids)) return e;
  }
  if (c->device < 0 || DEV_CHECKS) {  // host-only contexts: the index itself; development build: the device's, checked
    std::vector<gaml_aligment> buf;
    std::vector<AdviceSpan> spans;
    if (int e = advice_spans(c, *ps, 1, wids, nodes, buf, spans)) return e;
    advice_index_host(ps->mate[1].n_local(), spans, A.h_offs, A.h_ent);
    if (c->device < 0) A.n_ent = (int64_t)A.h_ent.size();
    else if (!advice_index_matches(c, *ps)) return fail(c, GAML_HIP_ESTATE, "advice: the device index differs from the host restatement");
  }
  A.built = true;
  A.threshold = threshold;
  return GAML_HIP_OK;
}

int ctx_advice_index(gaml_hip_ctx* c, int rs, std::vector<int64_t>& offs, std::vector<int32_t>& ent) {
  PairedSet* ps = nullptr;
  if (int e = advice_set(c, rs, &ps)) return e;
  const AdviceDev& A = ps->adv;
  if (!A.built) return fail(c, GAML_HIP_ESTATE, "advice: index not built (gaml_hip_advice_build)");
  if (c->device < 0) { offs = A.h_offs; ent = A.h_ent; return GAML_HIP_OK; }
  offs.resize((size_t)ps->mate[1].n_local() + 1);
  ent.resize((size_t)A.n_ent);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(offs.data(), A.offs.p, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (A.n_ent) HIP_TRY(c, hipMemcpy(ent.data(), A.ent.p, ent.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  return GAML_HIP_OK;
}

int ctx_advice_candidates(gaml_hip_ctx* c, int rs, const int32_t* path, int32_t n, const int32_t* reach, int32_t n_reach, int32_t flags,
                          const std::vector<int32_t>** list) {
  PairedSet* ps = nullptr;
  if (int e = advice_set(c, rs, &ps)) return e;
  AdviceDev& A = ps->adv;
  if (!A.built) return fail(c, GAML_HIP_ESTATE, "advice: index not built (gaml_hip_advice_build)");
  if (n < 0 || (n > 0 && !path) || n_reach < 0 || (n_reach > 0 && !reach) || (flags & ~3)) return fail(c, GAML_HIP_EINVAL, "advice: bad arguments");
  const int32_t nn = c->g.n();
  for (int32_t i = 0; i < n; i++) if (path[i] >= nn) return fail(c, GAML_HIP_EINVAL, "advice: path refers to a node outside the graph");
  for (int32_t i = 0; i < n_reach; i++) if (reach[i] < 0 || reach[i] >= nn) return fail(c, GAML_HIP_EINVAL, "advice: reach refers to a node outside the graph");
  ShortMate& m = ps->mate[0];
  register_for_contig(c->g, m, path, n);  // rs1.GetPositions: GetSubpathsFromPath + the precompute (graph.cc:667-672)
  if (int e = advice_align(c, *ps)) return e;
  advice_walk(c->g, m, path, n, A.steps);
  if (c->device >= 0) {
    if (int e = advice_query_dev(c, *ps, A.steps, path, n, reach, n_reach, flags, A.list)) return e;
  }
  if (c->device < 0 || DEV_CHECKS) {  // host-only contexts: the list itself; development build: the device's, checked
    std::vector<int32_t> wids, at, host_list;
    for (const AdviceStep& st : A.steps) { wids.push_back(st.wid); at.push_back(st.cur_pos); }
    std::vector<gaml_aligment> buf;
    std::vector<AdviceSpan> spans;
    if (int e = advice_spans(c, *ps, 0, wids, at, buf, spans)) return e;
    advice_candidates_host(m.n_local(), spans, A.h_offs, A.h_ent, path, n, reach, n_reach, flags, nn, c->device < 0 ? A.list : host_list);
    if (c->device >= 0 && host_list != A.list) return fail(c, GAML_HIP_ESTATE, "advice: the device's candidate list differs from the host restatement");
  }
  A.queries++;
  *list = &A.list;
  return GAML_HIP_OK;
}
}  // namespace gaml

extern "C" {

int gaml_hip_advice_build(gaml_hip_ctx* c, int readset, int32_t threshold) {
  MULTI_FWD(c, multi_advice_build(c->multi, readset, threshold));
  return ctx_advice_build(c, readset, threshold);
}

int64_t gaml_hip_advice_index(gaml_hip_ctx* c, int readset, int64_t* offs, int32_t* entries, int64_t cap) {
  MULTI_FWD(c, multi_advice_index(c->multi, readset, offs, entries, cap));
  std::vector<int64_t> o;
  std::vector<int32_t> e;
  if (int rc = ctx_advice_index(c, readset, o, e)) return rc;
  if (offs) std::copy(o.begin(), o.end(), offs);
  if (entries) std::copy(e.begin(), e.begin() + std::min<int64_t>(std::max<int64_t>(cap, 0), (int64_t)e.size()), entries);
  return (int64_t)e.size();
}

int64_t gaml_hip_advice_candidates(gaml_hip_ctx* c, int readset, const int32_t* path, int32_t path_len, const int32_t* reach, int32_t n_reach,
                                   int32_t flags, int32_t* out, int64_t cap) {
  MULTI_FWD(c, multi_advice_candidates(c->multi, readset, path, path_len, reach, n_reach, flags, out, cap));
  const std::vector<int32_t>* list = nullptr;
  if (int rc = ctx_advice_candidates(c, readset, path, path_len, reach, n_reach, flags, &list)) return rc;
  if (out) std::copy(list->begin(), list->begin() + std::min<int64_t>(std::max<int64_t>(cap, 0), (int64_t)list->size()), out);
  return (int64_t)list->size();
}

}  // extern "C"
