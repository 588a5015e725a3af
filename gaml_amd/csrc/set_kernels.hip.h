// set_kernels.hip.h -- the kernels beside the paired scorers: coverage sweeps, the single-end and PacBio scorers, a
// batch's per-set occurrence tables, bad_bases stores and the union of coverage maps.
#pragma once
#include "kernels.hip.h"
#include "paired_multi.hip.h"  // kMaxSets

namespace gaml {

// ---------------------------------------------------------------------------------------
// coverage penalty sweep (graph.cc:1893-1919) over the bitmap of marked path positions.
// A marked position p (not itself a contig start) adds p - q to bad_bases, q = previous marked
// position of the same path, when no contig start lies in (q, p], p - q > cov_move and
// p - (contig start before p) > mean + 5 sd.
// ---------------------------------------------------------------------------------------
struct CovArgs {
  const uint32_t* bits;
  const int* path_base;     // [n_paths+1] bit offsets (multiples of 32)
  const int* start_off;     // [n_paths+1] into starts
  const int* starts;        // contig start positions (path coordinates), ascending per path
  int n_paths;
  int total_words;
  double cov_move;
  double far;               // insert_mean + 5*insert_std
  unsigned long long* bad;  // out
};

// the words of one bitmap, strided over `blocks` blocks of which this is number `block`
__device__ __forceinline__ void coverage_sweep_words(const CovArgs& a, int block, int blocks) {
  for (int w = block * kBlock + threadIdx.x; w < a.total_words; w += blocks * kBlock) {
    uint32_t word = a.bits[w];
    if (!word) continue;
    // locate the path of this word (few paths: binary search)
    int lo = 0, hi = a.n_paths - 1;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (a.path_base[mid] <= w * 32) lo = mid; else hi = mid - 1; }
    const int base = a.path_base[lo], base_word = base >> 5;
    const int* st = a.starts + a.start_off[lo];
    const int nst = a.start_off[lo + 1] - a.start_off[lo];
    unsigned long long local = 0;
    uint32_t rest = word;
    while (rest) {
      const int b = __ffs(rest) - 1;
      rest &= rest - 1;
      const int p = w * 32 + b - base;
      // previous marked position q
      int q = -1;
      uint32_t below = word & ((1u << b) - 1);
      if (below) q = w * 32 + (31 - __clz(below)) - base;
      else {
        for (int v = w - 1; v >= base_word; v--) {
          uint32_t x = a.bits[v];
          if (x) { q = v * 32 + (31 - __clz(x)) - base; break; }
        }
      }
      if (q < 0) continue;  // previous event is the path start (type 1)
      // largest contig start <= p
      int l2 = 0, h2 = nst - 1;
      while (l2 < h2) { int mid = (l2 + h2 + 1) >> 1; if (st[mid] <= p) l2 = mid; else h2 = mid - 1; }
      const int lb = st[l2];
      if (lb > q) continue;  // a contig start in (q, p]: previous event has type 1 (or p is a start)
      if ((double)(p - q) > a.cov_move && (double)(p - lb) > a.far) local += (unsigned long long)(p - q);
    }
    if (local) atomicAdd(a.bad, local);
  }
}

__global__ __launch_bounds__(kBlock) void coverage_sweep_kernel(CovArgs a) { coverage_sweep_words(a, (int)blockIdx.x, (int)gridDim.x); }

// The sweeps of all path sets of a multi-set launch in ONE dispatch: blocks [block_off[s], block_off[s + 1]) sweep set s's
// bitmap into set s's counter (a set without a bit to sweep -- the empty assembly -- has no blocks: its counter stays 0).
struct CovMultiArgs { int n; int block_off[kMaxSets + 1]; CovArgs set[kMaxSets]; };
__global__ __launch_bounds__(kBlock) void coverage_sweep_multi_kernel(CovMultiArgs a) {
  int s = 0;
  while (s + 1 < a.n && (int)blockIdx.x >= a.block_off[s + 1]) s++;
  coverage_sweep_words(a.set[s], (int)blockIdx.x - a.block_off[s], a.block_off[s + 1] - a.block_off[s]);
}
// ... and their counters to where the host reads them after its wait (mapped pinned memory), n <= kMaxSets
__global__ void store_bad_multi_kernel(const unsigned long long* bad, unsigned long long* out, int n) {
  if (blockIdx.x == 0 && (int)threadIdx.x < n) out[threadIdx.x] = bad[threadIdx.x];
}

// ---------------------------------------------------------------------------------------
// single-end scorer (graph.cc:1650-1743): probs_i = sum over distinct absolute positions of
// m^e * M^(L-e); later record at the same position overwrites (graph.cc:633-644).
// ---------------------------------------------------------------------------------------
struct SingleArgs {
  MateView m;
  const int* lens;
  const double* floor_tab;     // exp(c + k*L)
  const double* logfloor_tab;
  double two_T;
  int n;
  double* probs;
  double* part_sum; int* part_zero; unsigned* ticket; double* out;
  double n_reads;
};

// One read under one path set's occurrence tables: the sum over its live candidates of m^e * M^(L-e). Shared by
// single_score_kernel and single_score_multi_kernel (same arithmetic in the same order: same bits).
__device__ __forceinline__ double single_read_acc(const MateView& m, const int4& r0, int L) {
  double acc = 0.0;
  // One record whose window occurs at most once in the scored paths -- nearly every read of an assembly without
  // repeats -- is its own only candidate: nothing can overwrite it (graph.cc:631-641), no second pass over the candidates.
  bool single_cand = false;
  if (r0.x >= 0 && ((unsigned)r0.z >> 9) == 0) {
    const int4 o = mate_occ(m, r0.x);
    if (o.z < 0) single_cand = true;  // the window is not part of the scored paths: the read scores nothing here
    else if (o.w >= 0) { single_cand = true; const int e = r0.z & 0xff; acc = m.mism_pow[e] * m.match_pow[L - e]; }
  }
  if (r0.x >= 0 && !single_cand) {
    for_each_cand(m, r0, [&](const Cand& x) {
      // positions are absolute here (path index * 1e6 folded into shift); all paths share one map
      bool live = true;
      for_each_cand(m, r0, [&](const Cand& d) {
        if (d.pos == x.pos && (d.rank > x.rank || (d.rank == x.rank && d.k > x.k))) live = false;
      });
      if (live) acc += m.mism_pow[x.edit] * m.match_pow[L - x.edit];
    });
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void single_score_kernel(SingleArgs a) {
  __shared__ double sh_s[kBlock / 64];
  __shared__ int sh_z[kBlock / 64];
  double lsum = 0.0;
  int zeros = 0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const int4 r0 = a.m.first[i];
    const int L = a.lens[i];
    const double acc = single_read_acc(a.m, r0, L);
    a.probs[i] = acc;
    const double p = acc / a.two_T;  // GetTotalProb single (graph.cc:1526-1534)
    if (p < a.floor_tab[L]) { zeros++; lsum += a.logfloor_tab[L]; }
    else lsum += log(p);
  }
  block_reduce(lsum, zeros, sh_s, sh_z);
  // bad_bases of the single-end scorer is identically 0 (graph.cc:1701-1733)
  grid_finish(lsum, zeros, blockIdx.x, gridDim.x, a.part_sum, a.part_zero, a.ticket, a.out, 0.0, a.n_reads, sh_s, sh_z);
}

// ---------------------------------------------------------------------------------------
// PacBio scorer (graph.cc:3052-3088, 3223): per read log-sum-exp over its cached alignments,
// each counted once per occurrence of its sub-walk in the scored paths; floor; sum.
// One WAVE per read: lanes stride over the read's records (coalesced 8-B logprob loads),
// each lane folds its share with the reference's pairwise rule max + log1p(exp(min-max)),
// then the 64 partial values are combined by a butterfly of the same rule.
// ---------------------------------------------------------------------------------------
struct PacbioArgs {
  const int* rec_off;        // [n+1] read-major CSR
  const int* rec_walk;       // sub-walk id per record
  const double* rec_logp;    // log probability per record
  const int* walk_count;     // occurrences of each sub-walk in the scored paths
  const int* lens;
  double floor_a, floor_b;   // log(exp(min_prob_start)), log(exp(min_prob_per_base)) (graph.cc:3075-3076)
  int n;
  double* logprobs;          // out: per-read log probability (-inf when no alignment)
  double* part_sum; int* part_zero; unsigned* ticket; double* out;
  double n_reads, bad_bases;
};

__device__ __forceinline__ double lse2(double a, double b) {  // logdouble operator+ (logdouble.hpp:37-47)
  const double ninf = -__builtin_huge_val();
  if (a == ninf) return b;
  if (b == ninf) return a;
  const double hi = fmax(a, b), lo = fmin(a, b);
  return hi + log1p(exp(lo - hi));
}

__global__ __launch_bounds__(kBlock) void pacbio_score_kernel(PacbioArgs a) {
  __shared__ double sh_s[kBlock / 64];
  __shared__ int sh_z[kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int wave_global = (blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int n_waves = (gridDim.x * kBlock) >> 6;
  double lsum = 0.0;
  int zeros = 0;
  for (int i = wave_global; i < a.n; i += n_waves) {
    const int b = a.rec_off[i], e = a.rec_off[i + 1];
    double v = -__builtin_huge_val();
    for (int k = b + lane; k < e; k += 64) {
      const int c = a.walk_count[a.rec_walk[k]];
      const double lp = a.rec_logp[k];
      for (int t = 0; t < c; t++) v = lse2(v, lp);
    }
    for (int off = 32; off > 0; off >>= 1) v = lse2(v, __shfl_xor(v, off, 64));
    if (lane == 0) {
      a.logprobs[i] = v;
      const double floor_lp = a.floor_a + a.floor_b * (double)a.lens[i];
      if (v < floor_lp) { zeros++; v = floor_lp; }
      lsum += v;
    }
  }
  block_reduce(lsum, zeros, sh_s, sh_z);
  grid_finish(lsum, zeros, blockIdx.x, gridDim.x, a.part_sum, a.part_zero, a.ticket, a.out, a.bad_bases, a.n_reads, sh_s, sh_z);
}

// The end of a multi-set scoring kernel (pacbio_score_multi_kernel, single_score_multi_kernel): block_reduce and grid_finish
// per set, in their order, with rows of partials of the sets' own (set s, block b: [s * part_stride + b]) and ONE ticket for
// all sets; out[4 s ..] = {sum, floored, 0, reads}. Every loop over the sets is unrolled over kMaxSets: lsum / zeros stay
// in registers.
__device__ __forceinline__ void multi_grid_finish(double (&lsum)[kMaxSets], int (&zeros)[kMaxSets], int n_sets, double* part_sum, int* part_zero,
                                                  int part_stride, unsigned* ticket, double* out, double n_reads,
                                                  double (&sh_s)[kMaxSets][kBlock / 64], int (&sh_z)[kMaxSets][kBlock / 64]) {
  __shared__ bool is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // block_reduce per set, into rows of their own: one barrier for all sets
#pragma unroll
  for (int s = 0; s < kMaxSets; s++)
    if (s < n_sets) {
      for (int off = 32; off > 0; off >>= 1) {
        lsum[s] += __shfl_down(lsum[s], off, 64);
        zeros[s] += __shfl_down(zeros[s], off, 64);
      }
      if (lane == 0) { sh_s[s][wave] = lsum[s]; sh_z[s][wave] = zeros[s]; }
    }
  __syncthreads();
  // grid_finish with ONE ticket for all sets (its `is_last` is one word: called once per set, thread 0 of the next call
  // could overwrite it before a slow wave has read the previous value)
  const int n_partials = (int)gridDim.x, my_slot = (int)blockIdx.x;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < kMaxSets; s++)
      if (s < n_sets) {
        double ts = 0; int tz = 0;
        for (int w = 0; w < kBlock / 64; w++) { ts += sh_s[s][w]; tz += sh_z[s][w]; }
        __hip_atomic_store(&part_sum[(size_t)s * part_stride + my_slot], ts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part_zero[(size_t)s * part_stride + my_slot], tz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int g = my_slot & 15;
    const unsigned in_group = (unsigned)((n_partials - g + 15) >> 4), groups = (unsigned)min(16, n_partials);
    bool last = false;
    if (__hip_atomic_fetch_add(&ticket[1 + g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_group - 1)
      last = __hip_atomic_fetch_add(&ticket[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
    is_last = last;
  }
  __syncthreads();
  if (!is_last) return;
#pragma unroll
  for (int s = 0; s < kMaxSets; s++)
    if (s < n_sets) {
      double ts = 0; int tz = 0;
      for (int b = threadIdx.x; b < n_partials; b += kBlock) {
        ts += __hip_atomic_load(&part_sum[(size_t)s * part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tz += __hip_atomic_load(&part_zero[(size_t)s * part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      for (int off = 32; off > 0; off >>= 1) {
        ts += __shfl_down(ts, off, 64);
        tz += __shfl_down(tz, off, 64);
      }
      if (lane == 0) { sh_s[s][wave] = ts; sh_z[s][wave] = tz; }  // (thread 0 read the rows before the barrier above)
    }
  __syncthreads();
  if (threadIdx.x < kTicketWords) __hip_atomic_store(&ticket[threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < kMaxSets; s++)
      if (s < n_sets) {
        double ts = 0; int tz = 0;
        for (int w = 0; w < kBlock / 64; w++) { ts += sh_s[s][w]; tz += sh_z[s][w]; }
        out[4 * s] = ts; out[4 * s + 1] = (double)tz; out[4 * s + 2] = 0.0; out[4 * s + 3] = n_reads;
      }
  }
}

// The same for up to kMaxSets path sets in one pass over the records (gaml_hip_calc_prob_batch, pacbio_batch.hip.h): a
// record's sub-walk id and log probability are loaded once, the sets' occurrence counts of that sub-walk stand side by
// side in `counts` (32 bytes per sub-walk: two 16-byte loads). Same grid, same read-to-wave mapping, same fold order and
// the same finishing arithmetic as pacbio_score_kernel, per set: every set's four partials are the bits a call of its own
// would give. The per-set values live in registers: every loop over the sets is unrolled over the compile-time kMaxSets
// with the guard s < n_sets, no array is indexed at run time.
struct PacbioMultiArgs {
  const int* rec_off; const int* rec_walk; const double* rec_logp;
  const int* counts;         // [sub-walk][kMaxSets]; columns >= n_sets hold 0
  const int* lens;
  double floor_a, floor_b;
  int n, n_sets;
  double* logprobs;          // out: per-read log probability under the LAST set (what sequential calls leave there)
  double* part_sum; int* part_zero;  // set s, block b: [s * part_stride + b]
  int part_stride;
  unsigned* ticket;          // kTicketWords, one ticket for all sets
  double* out;               // set s: out[4 s ..] = {sum, floored, 0, reads}
  double n_reads;
};

__global__ __launch_bounds__(kBlock) void pacbio_score_multi_kernel(PacbioMultiArgs a) {
  __shared__ double sh_s[kMaxSets][kBlock / 64];
  __shared__ int sh_z[kMaxSets][kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int wave_global = (blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int n_waves = (gridDim.x * kBlock) >> 6;
  double lsum[kMaxSets];
  int zeros[kMaxSets];
#pragma unroll
  for (int s = 0; s < kMaxSets; s++) { lsum[s] = 0.0; zeros[s] = 0; }
  for (int i = wave_global; i < a.n; i += n_waves) {
    const int b = a.rec_off[i], e = a.rec_off[i + 1];
    double v[kMaxSets];
#pragma unroll
    for (int s = 0; s < kMaxSets; s++) v[s] = -__builtin_huge_val();
    for (int k = b + lane; k < e; k += 64) {
      const int4* cp = (const int4*)(a.counts + (size_t)a.rec_walk[k] * kMaxSets);
      const int4 c0 = cp[0], c1 = cp[1];
      const int cnt[kMaxSets] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const double lp = a.rec_logp[k];
#pragma unroll
      for (int s = 0; s < kMaxSets; s++)
        if (s < a.n_sets) for (int t = 0; t < cnt[s]; t++) v[s] = lse2(v[s], lp);
    }
#pragma unroll
    for (int s = 0; s < kMaxSets; s++)
      if (s < a.n_sets) for (int off = 32; off > 0; off >>= 1) v[s] = lse2(v[s], __shfl_xor(v[s], off, 64));
    if (lane == 0) {
      const double floor_lp = a.floor_a + a.floor_b * (double)a.lens[i];
#pragma unroll
      for (int s = 0; s < kMaxSets; s++)
        if (s < a.n_sets) {
          double x = v[s];
          if (s == a.n_sets - 1) a.logprobs[i] = x;
          if (x < floor_lp) { zeros[s]++; x = floor_lp; }
          lsum[s] += x;
        }
    }
  }
  multi_grid_finish(lsum, zeros, a.n_sets, a.part_sum, a.part_zero, a.part_stride, a.ticket, a.out, a.n_reads, sh_s, sh_z);
}

// The single-end scorer for up to kMaxSets path sets in one pass over the read-major records (gaml_hip_calc_prob_batch,
// single_batch.hip.h): a read's first record and length are loaded once; every set brings occurrence tables of its own (the
// three pointers of a MateView, into one arena) and its 2T. The record table holds the windows of ALL sets of the chunk: a
// window a set does not name reads as absent in that set's table and is skipped, the candidates that remain keep their
// (record, occurrence) order, so single_read_acc adds the terms a launch of single_score_kernel for that set alone adds,
// in its order. Same grid and read-to-thread mapping; finished like pacbio_score_multi_kernel. The rule of that kernel
// holds here too: per-set pointers are fixed arrays of kMaxSets in the arguments, every loop over the sets is unrolled over
// the compile-time kMaxSets with the guard s < n_sets, no array is indexed at run time.
struct SingleMultiArgs {
  const int4* first; const int4* extra;             // MateView: what does not depend on the path set
  const double* mism_pow; const double* match_pow;
  const int* lens;
  const double* floor_tab; const double* logfloor_tab;
  int n, n_sets;
  const int4* occ[kMaxSets]; const int* multi_off[kMaxSets]; const int4* multi[kMaxSets];  // MateView: set s's tables
  double two_T[kMaxSets];
  double* probs;             // out: per-read value under the LAST set (what sequential calls leave there)
  double* part_sum; int* part_zero;  // set s, block b: [s * part_stride + b]
  int part_stride;
  unsigned* ticket;          // kTicketWords, one ticket for all sets
  double* out;               // set s: out[4 s ..] = {sum, floored, 0, reads} (bad_bases is identically 0: single_score_kernel)
  double n_reads;
};

__global__ __launch_bounds__(kBlock) void single_score_multi_kernel(SingleMultiArgs a) {
  __shared__ double sh_s[kMaxSets][kBlock / 64];
  __shared__ int sh_z[kMaxSets][kBlock / 64];
  double lsum[kMaxSets];
  int zeros[kMaxSets];
#pragma unroll
  for (int s = 0; s < kMaxSets; s++) { lsum[s] = 0.0; zeros[s] = 0; }
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const int4 r0 = a.first[i];
    const int L = a.lens[i];
    const double floor_p = a.floor_tab[L], floor_lp = a.logfloor_tab[L];
#pragma unroll
    for (int s = 0; s < kMaxSets; s++)
      if (s < a.n_sets) {
        const MateView m{a.first, a.extra, a.occ[s], nullptr, a.multi_off[s], a.multi[s], a.mism_pow, a.match_pow};
        const double acc = single_read_acc(m, r0, L);
        if (s == a.n_sets - 1) a.probs[i] = acc;
        const double p = acc / a.two_T[s];  // GetTotalProb single (graph.cc:1526-1534)
        if (p < floor_p) { zeros[s]++; lsum[s] += floor_lp; }
        else lsum[s] += log(p);
      }
  }
  multi_grid_finish(lsum, zeros, a.n_sets, a.part_sum, a.part_zero, a.part_stride, a.ticket, a.out, a.n_reads, sh_s, sh_z);
}

// ---------------------------------------------------------------------------------------------------------
// A batch's per-set occurrence tables, built on the device: set g = the resident tables (the path set of the
// previous call) + the entries that changed from set to set, patches of sets 0..g applied in order. The host
// writes only the patches (a few dozen 16-byte entries per candidate) instead of every set's whole tables.
// ---------------------------------------------------------------------------------------------------------
struct BatchPatch { int32_t w; uint32_t lo, hi; int32_t rank; };  // table entry w := {lo, hi, rank}
struct BatchTabArgs {
  const char* base;      // the resident tables
  char* regions;         // set g at regions + g * stride, laid out like the resident tables
  size_t stride;
  size_t off_occ[2], bytes_occ[2], off_lo[2], bytes_lo[2], off_m[2], bytes_m[2];  // per mate; byte counts are multiples of 4
  const BatchPatch* patches;
  const int* patch_off;  // patches of (set g, mate mt): [patch_off[2 g + mt], patch_off[2 g + mt + 1])
  int first;             // first set of this launch
  int n_sets;            // sets of this launch
  unsigned char* chg[2]; // per mate: MultiSets::chg of this launch (one byte per table entry), written by the last blocks
  size_t chg_bytes[2];   // multiples of 16
};

__device__ __forceinline__ void block_copy_words(char* dst, const char* src, size_t bytes) {  // both 16-byte aligned
  const size_t n16 = bytes / 16;
  for (size_t i = threadIdx.x; i < n16; i += blockDim.x) ((int4*)dst)[i] = ((const int4*)src)[i];
  const size_t done = n16 * 16;
  for (size_t i = done / 4 + threadIdx.x; i < bytes / 4; i += blockDim.x) ((int*)dst)[i] = ((const int*)src)[i];
}

__global__ __launch_bounds__(1024) void batch_tables_kernel(BatchTabArgs a) {  // grid (sets of this launch + 1, 2 mates)
  const int mt = (int)blockIdx.y;
  if ((int)blockIdx.x == a.n_sets) {
    // which of this launch's sets may differ from its first one, per table entry: set s differs in the entries its own
    // patch and the patches of the sets between them name -- bits s .. n-1 for every entry of patch first + s
    int4* z = (int4*)a.chg[mt];
    for (size_t i = threadIdx.x; i < a.chg_bytes[mt] / 16; i += blockDim.x) z[i] = make_int4(0, 0, 0, 0);
    __syncthreads();
    for (int sidx = 1; sidx < a.n_sets; sidx++) {
      const unsigned bits = (0xffu << sidx) & 0xffu;
      for (int t = a.patch_off[2 * (a.first + sidx) + mt] + (int)threadIdx.x; t < a.patch_off[2 * (a.first + sidx) + mt + 1]; t += blockDim.x) {
        const int w = a.patches[t].w;
        atomicOr((unsigned*)(a.chg[mt] + (w & ~3)), bits << (8 * (w & 3)));
      }
    }
    return;
  }
  const int g = a.first + (int)blockIdx.x;
  char* region = a.regions + (size_t)g * a.stride;
  block_copy_words(region + a.off_occ[mt], a.base + a.off_occ[mt], a.bytes_occ[mt]);
  block_copy_words(region + a.off_lo[mt], a.base + a.off_lo[mt], a.bytes_lo[mt]);
  block_copy_words(region + a.off_m[mt], a.base + a.off_m[mt], a.bytes_m[mt]);
  int* occ = (int*)(region + a.off_occ[mt]);
  for (int j = 0; j <= g; j++) {  // later sets override earlier ones
    __syncthreads();
    for (int t = a.patch_off[2 * j + mt] + (int)threadIdx.x; t < a.patch_off[2 * j + mt + 1]; t += blockDim.x) {
      const BatchPatch pt = a.patches[t];
      int* e = occ + 3 * (size_t)pt.w;
      e[0] = (int)pt.lo; e[1] = (int)pt.hi; e[2] = pt.rank;
    }
  }
}

// bad_bases of a paired set with coverage penalty: u64 counter of the sweep -> its partial slot
// (scale 0: a rank other than 0 of a sharded evaluation -- the all-reduce(sum) of the partials must
// count the value once)
__global__ void store_bad_bases_kernel(const unsigned long long* bad, double* out4, double scale) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out4[2] = scale * (double)*bad;
}

// union of the coverage maps of all ranks: own |= maps[0] | maps[1] | ...
__global__ __launch_bounds__(kBlock) void or_maps_kernel(uint32_t* own, const uint32_t* maps, int n_maps, int words) {
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < words; w += gridDim.x * kBlock) {
    uint32_t v = own[w];
    for (int k = 0; k < n_maps; k++) v |= maps[(size_t)k * words + w];
    own[w] = v;
  }
}

}  // namespace gaml
