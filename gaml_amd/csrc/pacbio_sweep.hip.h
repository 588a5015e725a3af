// pacbio_sweep.hip.h -- the coverage sweep of CalcScoreForPacbio (graph.cc:3198-3250) on the device.
//
// The reference sorts (position, +1 | begin - end) events of every contig's node intervals, the fixed interval
// (-1000, 2000) and the alignment intervals of all records that clear GetMinReadProb, walks them with a multiset of
// the open intervals' begins, and after every event j adds
//     max(0, min(next event's position, tl - 250, open.empty() ? tl - 250 : int(min(open) + step)) - max(2500, position_j))
// to bad_bases. Every interval has end > begin (an event with value +1 is an opening; closing an interval that is not
// open is undefined in the reference, graph.cc:3229-3231), so closings at a position come before its openings, every
// closing finds its opening, and only the LAST event of a position contributes (for the others the next event is at
// the same position). After all events at position p the open intervals are exactly those with begin <= p < end, and
// with the intervals ordered by begin the one with the smallest begin among them is the first whose running maximum
// of `end` exceeds p (all before it have closed; if it begins after p nothing is open). Hence, without a multiset:
//   1. sort the intervals by (contig, begin); running maximum of (contig, end) over that order (segmented by contig
//      for free: the contig is the key's high word);
//   2. sort all begins and ends by (contig, position);
//   3. one thread per sorted position: skip it when the next one is equal; binary search of the running maxima for
//      the open interval with the smallest begin; the term above; block sums, one atomic add per block.
// Integer arithmetic throughout (int(min + step) truncates a double exactly as the reference's int = int + double):
// bad_bases equals the reference's sweep bit for bit. HBM traffic: 16 B per interval in, ~100 B per interval through
// the two radix sorts -- a few hundred KB per evaluation; the launches' latency is what it costs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gaml {

// one occurrence of a cached sub-walk in a path of the evaluation
struct PbOcc {
  int32_t walk;  // cache id: intervals iv[iv_off[walk] .. iv_off[walk + 1])
  int32_t base;  // path position of the sub-walk's first base (graph.cc:2498)
  int32_t path;  // contig number in this evaluation
  int32_t out;   // first slot of its intervals in the evaluation's interval list
};

// (contig, position) as one ascending unsigned key; positions may be negative (-1000)
__device__ __forceinline__ unsigned long long pb_key(int path, int pos) {
  return ((unsigned long long)(unsigned)path << 32) | (unsigned long long)((unsigned)pos ^ 0x80000000u);
}
__device__ __forceinline__ int pb_key_path(unsigned long long k) { return (int)(unsigned)(k >> 32); }
__device__ __forceinline__ int pb_key_pos(unsigned long long k) { return (int)(((unsigned)k) ^ 0x80000000u); }

// the alignment intervals of every occurrence, in path coordinates: {contig, begin, end, 0}. One wavefront per occurrence.
__global__ __launch_bounds__(256) void pacbio_intervals_kernel(const PbOcc* __restrict__ occ, int n_occ, const int* __restrict__ iv_off,
                                                                const int2* __restrict__ iv, int4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int waves = (gridDim.x * blockDim.x) >> 6;
  for (int o = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; o < n_occ; o += waves) {
    const PbOcc oc = occ[o];
    const int first = iv_off[oc.walk], n = iv_off[oc.walk + 1] - first;
    for (int t = lane; t < n; t += 64) {
      const int2 v = iv[first + t];
      out[oc.out + t] = make_int4(oc.path, oc.base + v.x, oc.base + v.y, 0);
    }
  }
}

__global__ __launch_bounds__(256) void pacbio_sweep_keys_kernel(const int4* __restrict__ iv, int n, unsigned long long* __restrict__ key_begin,
                                                                 unsigned long long* __restrict__ key_end, unsigned long long* __restrict__ pos) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const int4 v = iv[k];
    const unsigned long long b = pb_key(v.x, v.y), e = pb_key(v.x, v.z);
    key_begin[k] = b;
    key_end[k] = e;
    pos[2 * k] = b;
    pos[2 * k + 1] = e;
  }
}

// pos: the 2n begins and ends sorted; key_begin: the n intervals' begins sorted; end_max: running maximum of their
// (contig, end) keys in that order; tl: contig lengths (GetReadProbabilities' total_len, graph.cc:2431)
// PER_CONTIG: every term goes into bad[contig] instead of the one word (the batch's contigs above the block-per-contig
// kernel's capacity, pacbio_path_sweep_kernel below; integer atomics: the order does not matter)
template <bool PER_CONTIG>
__global__ __launch_bounds__(256) void pacbio_sweep_kernel(const unsigned long long* __restrict__ pos, int n2,
                                                            const unsigned long long* __restrict__ key_begin,
                                                            const unsigned long long* __restrict__ end_max, int n, const int* __restrict__ tl,
                                                            double step, unsigned long long* __restrict__ bad) {
  __shared__ unsigned long long sh[4];
  unsigned long long mine = 0;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += gridDim.x * blockDim.x) {
    const unsigned long long here = pos[j];
    const bool has_next = j + 1 < n2;
    const unsigned long long nxt = has_next ? pos[j + 1] : 0ull;
    if (has_next && nxt == here) continue;  // not the last event of its position
    const int q = pb_key_path(here), p = pb_key_pos(here);
    int good = tl[q] - 250;
    // the open interval with the smallest begin: first interval whose running maximum of `end` exceeds p
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (end_max[mid] > here) hi = mid; else lo = mid + 1;
    }
    if (lo < n) {
      const unsigned long long kb = key_begin[lo];
      if (pb_key_path(kb) == q && pb_key_pos(kb) <= p) good = (int)((double)pb_key_pos(kb) + step);  // int = int + double (graph.cc:3236)
    }
    if (has_next && pb_key_path(nxt) == q) good = min(pb_key_pos(nxt), good);
    good = min(good, tl[q] - 250);
    const int from = max(2500, p);
    if (good > from) {
      if (PER_CONTIG) atomicAdd(bad + q, (unsigned long long)(good - from));
      else mine += (unsigned long long)(good - from);
    }
  }
  if (PER_CONTIG) return;
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = sh[0] + sh[1] + sh[2] + sh[3];
    if (total) atomicAdd(bad, total);
  }
}

// ---------------------------------------------------------------------------------------------------------
// The sweep of ONE contig by ONE block (the PacBio side of the batch's one-pass routes, pacbio_batch.hip.h): bad_bases of a
// call is a sum over its paths (graph.cc:3183-3251), and a path's events depend on the path and the record cache alone, so
// a chunk sweeps every path it has no value for once, each on its own. A contig's intervals fit LDS: gathered there, ordered
// by a bitonic network, running maximum, the 2n positions ordered the same way, the term of pacbio_sweep_kernel per
// position, block sum, one plain 64-bit store. Positions are contig-local: keys are 32-bit (the sign bit flipped, so that
// unsigned order is signed order), an interval is (begin << 32 | end) -- ordered by begin; which of several intervals with
// one begin comes first does not change the first index whose running maximum exceeds a position, nor the begin found there.
// No global sort, no atomics, no scratch. Every index is checked against the header's and the launch's counts before it is
// used; a header that does not add up stores ~0 (the host refuses the chunk).
// ---------------------------------------------------------------------------------------------------------
constexpr int kPbSweepCap = 2048;  // intervals per contig: 8 B per interval + 2 x 4 B per position = 32 KB of LDS per block

struct PbPathHdr {
  int32_t tl;               // the contig's length (GetReadProbabilities' total_len)
  int32_t node_off, n_node; // its node intervals {begin, end}, the fixed (-1000, 2000) first: node[node_off .. node_off + n_node)
  int32_t occ_off, n_occ;   // its cached sub-walks: occ[occ_off .. occ_off + n_occ)
  int32_t n_iv;             // intervals in all: n_node + the records' of every occurrence
  int32_t out;              // slot of its bad_bases in the result array
  int32_t pad;
};
struct PbPathOcc {
  int32_t walk;  // cache id: intervals iv[iv_off[walk] .. iv_off[walk + 1])
  int32_t base;  // path position of the sub-walk's first base
  int32_t out;   // first slot of its intervals among the contig's n_iv
  int32_t pad;
};
struct PbPathSweepArgs {
  const PbPathHdr* hdr;  // one per block
  const int2* node; int n_node_all;
  const PbPathOcc* occ; int n_occ_all;
  const int* iv_off; int n_walks;  // PbSweepDev's walk-major intervals
  const int2* iv; int n_iv_all;
  double step;
  unsigned long long* bad; int n_bad;
};

__device__ __forceinline__ unsigned pb_flip(int v) { return (unsigned)v ^ 0x80000000u; }

// ascending bitonic network over a[0 .. P), P a power of two, by the whole block; ends with a barrier. A thread owns one
// compare-exchange per step: strides of 32 elements and more touch consecutive addresses (no bank conflict), the five
// smaller strides of every merge cost a 2-way one.
template <class T>
__device__ __forceinline__ void pb_bitonic(T* a, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += 256) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const T x = a[lo], y = a[hi];
        if ((x > y) == ((lo & k) == 0)) { a[lo] = y; a[hi] = x; }
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pacbio_path_sweep_kernel(PbPathSweepArgs a) {
  __shared__ unsigned long long iv[kPbSweepCap];  // (begin, end), flipped; after the scan (begin, running maximum of the ends)
  __shared__ unsigned pos[2 * kPbSweepCap];
  __shared__ unsigned wave_max[4];
  __shared__ unsigned long long wave_sum[4];
  __shared__ int refused;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PbPathHdr h = a.hdr[blockIdx.x];
  const int n = h.n_iv;
  if (h.out < 0 || h.out >= a.n_bad) return;  // (nowhere to say so)
  const bool hdr_ok = n >= 1 && n <= kPbSweepCap && h.n_node >= 0 && h.n_node <= n && h.node_off >= 0 && h.node_off <= a.n_node_all - h.n_node &&
                      h.n_occ >= 0 && h.occ_off >= 0 && h.occ_off <= a.n_occ_all - h.n_occ;
  if (!hdr_ok) { if (threadIdx.x == 0) a.bad[h.out] = ~0ull; return; }
  int P = 2;
  while (P < n) P <<= 1;
  if (threadIdx.x == 0) refused = 0;
  for (int i = threadIdx.x; i < P; i += 256) iv[i] = ~0ull;
  __syncthreads();
  // 1. the contig's intervals: its nodes', then one wavefront per occurrence for the records'
  for (int t = threadIdx.x; t < h.n_node; t += 256) {
    const int2 v = a.node[h.node_off + t];
    iv[t] = ((unsigned long long)pb_flip(v.x) << 32) | pb_flip(v.y);
  }
  for (int o = wave; o < h.n_occ; o += 4) {
    const PbPathOcc oc = a.occ[h.occ_off + o];
    bool ok = oc.walk >= 0 && oc.walk < a.n_walks;
    int first = 0, cnt = 0;
    if (ok) {
      first = a.iv_off[oc.walk];
      cnt = a.iv_off[oc.walk + 1] - first;
      ok = first >= 0 && cnt >= 0 && first <= a.n_iv_all - cnt && oc.out >= h.n_node && oc.out <= n - cnt;
    }
    if (!ok) { if (lane == 0) refused = 1; continue; }
    for (int t = lane; t < cnt; t += 64) {
      const int2 v = a.iv[first + t];
      iv[oc.out + t] = ((unsigned long long)pb_flip(oc.base + v.x) << 32) | pb_flip(oc.base + v.y);
    }
  }
  __syncthreads();
  if (refused) { if (threadIdx.x == 0) a.bad[h.out] = ~0ull; return; }
  // 2. by begin
  pb_bitonic(iv, P);
  for (int i = threadIdx.x; i < P; i += 256) {
    const unsigned long long v = iv[i];
    const bool real = i < n;
    pos[2 * i] = real ? (unsigned)(v >> 32) : ~0u;
    pos[2 * i + 1] = real ? (unsigned)v : ~0u;
  }
  // 3. running maximum of the ends: a thread owns P / 256 consecutive intervals; their maxima are scanned per wave by
  //    shuffles, across the four waves through LDS
  const int per = P >= 256 ? P / 256 : 1, mine0 = (int)threadIdx.x * per;
  unsigned top = 0;  // (flipped keys: 0 is below every position)
  for (int i = mine0; i < mine0 + per && i < n; i++) top = max(top, (unsigned)iv[i]);
  unsigned incl = top;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned u = __shfl_up(incl, off, 64);
    if (lane >= off) incl = max(incl, u);
  }
  if (lane == 63) wave_max[wave] = incl;
  __syncthreads();  // (also: pos is written)
  unsigned run = __shfl_up(incl, 1, 64);
  if (lane == 0) run = 0;
  for (int w = 0; w < wave; w++) run = max(run, wave_max[w]);
  for (int i = mine0; i < mine0 + per && i < n; i++) {
    const unsigned long long v = iv[i];
    run = max(run, (unsigned)v);
    iv[i] = (v & 0xffffffff00000000ull) | run;
  }
  // 4. the 2n begins and ends (the padding sorts behind them)
  pb_bitonic(pos, 2 * P);
  // 5. the term of pacbio_sweep_kernel per position
  unsigned long long sum = 0;
  const int n2 = 2 * n, cap = h.tl - 250;
  for (int j = threadIdx.x; j < n2; j += 256) {
    const unsigned here = pos[j];
    const bool has_next = j + 1 < n2;
    const unsigned nxt = has_next ? pos[j + 1] : 0u;
    if (has_next && nxt == here) continue;  // not the last event of its position
    const int p = (int)(here ^ 0x80000000u);
    int good = cap;
    int lo = 0, hi = n;  // the open interval with the smallest begin: first whose running maximum of `end` exceeds p
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((unsigned)iv[mid] > here) hi = mid; else lo = mid + 1;
    }
    if (lo < n) {
      const int b = (int)((unsigned)(iv[lo] >> 32) ^ 0x80000000u);
      if (b <= p) good = (int)((double)b + a.step);  // int = int + double (graph.cc:3236)
    }
    if (has_next) good = min((int)(nxt ^ 0x80000000u), good);
    good = min(good, cap);
    const int from = max(2500, p);
    if (good > from) sum += (unsigned long long)(good - from);
  }
  // 6. / 7. block sum, one plain store
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) wave_sum[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) a.bad[h.out] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// the chunk's per-contig values to where the host reads them after its wait (mapped pinned memory)
__global__ __launch_bounds__(256) void pacbio_store_bad_kernel(const unsigned long long* __restrict__ bad, unsigned long long* __restrict__ out, int n) {
  for (int k = threadIdx.x; k < n; k += 256) out[k] = bad[k];
}

}  // namespace gaml
