// paired_multi.hip.h -- the paired scorer for several path sets in one pass over the records (paired_score_multi_kernel)
// and the callees of the pairs on repeated windows (compact_general_call, general_pair_call), which read either
// launch's argument block. The single-set kernel, the shared types and the class bodies it repeats: kernels.hip.h.
#pragma once
#include "kernels.hip.h"

namespace gaml {

// ---------------------------------------------------------------------------------------------------------
// Several path sets in ONE pass over the records (gaml_hip_calc_prob_batch; the move generators compare a handful of
// near-identical candidate assemblies: moves.cc:107-113 LocalChange2, 694-800 FixGapLength, 1156-1305 FixRepForNode2).
// A path set only changes WHERE windows sit (its occurrence tables, 12 B per window) and 2T; the records, the
// memo of pair terms and the grid are the same for all of them. So: the compact class (90 % of the pairs) loads
// its 8-byte records once and resolves them against every set's tables (S x 95 KB at cfg3: L2 resident) in an inner
// loop; the other classes (10 % of the pairs, a few records each, L2 hits after the first set) simply run their body
// once per set. Every (block, set) writes its own partial: same lane -> pair mapping and reduction order as the
// single-set kernel, so a batch gives bit for bit what the sets give one by one.
// ---------------------------------------------------------------------------------------------------------
constexpr int kMaxSets = 8;
struct SetDev {  // what differs between the path sets of one batch
  const Occ12* occ12[2];
  const int* multi_off[2];
  const int4* multi[2];
  const double* tfloor_c;          // [code] for this set's 2T
  double tfloor0;                  // = tfloor_c[0], by value
  double two_T, log_two_T;
  double* part_sum;                // this set's per-block partials
  int* part_zero;
  // a set with a coverage penalty: its own bitmap (a region of the launch's buffer at a 32-bit-aligned offset) and its own
  // slot_base table -- PairedArgs::cov_bits / path_base of a single call; null for a set without penalty
  uint32_t* cov_bits;
  const int* slot_base;
};
// chg[mt][w]: bit s set = window w's table entry in set s of this launch may differ from set 0's (s >= 1; a batch whose
// sets' tables were built from patches knows, batch_tables_kernel). A pair none of whose records touch such a window
// resolves to the same candidates in set s as in set 0: its set-0 result is finished again under set s's 2T and
// thresholds, no table is read. The bits are cumulative (bit s implies bit s + 1: a set's tables are its
// predecessor's plus a patch). Null: unknown, every set resolves every pair. Used by the classes with several records
// per pair and the delta / wave-per-pair blocks; the compact class resolves every set (see its body).
struct MultiSets { int n; int skip_classes; const unsigned char* chg[2]; SetDev set[kMaxSets]; };

constexpr int kTfCodes = 16;  // length codes whose per-set thresholds a multi-set block keeps in LDS
// COV: the launch marks coverage -- the set's bitmap and slot_base table travel too (pair_term, compact_cover and the general
// paths then mark into this set's bitmap); without it the view is what it always was
template <bool COV = false>
__device__ __forceinline__ PairedArgs with_set(const PairedArgs& a, const SetDev& sd, const double* tfloor_lds = nullptr) {
  PairedArgs b = a;
  if (COV) { b.cov_bits = sd.cov_bits; b.path_base = sd.slot_base; }
#pragma unroll
  for (int mt = 0; mt < 2; mt++) { b.m[mt].occ12 = sd.occ12[mt]; b.occ12[mt] = sd.occ12[mt]; b.m[mt].multi_off = sd.multi_off[mt]; b.m[mt].multi = sd.multi[mt]; }
  b.tfloor_c = tfloor_lds ? tfloor_lds : sd.tfloor_c; b.tfloor0 = sd.tfloor0; b.two_T = sd.two_T; b.log_two_T = sd.log_two_T;
  b.part_sum = sd.part_sum; b.part_zero = sd.part_zero;
  return b;
}

// the kernel's argument block, read where it is needed (a callee's view of it); a multi-set launch's: {PairedArgs, MultiSets}
struct MultiKernArgs { PairedArgs a; MultiSets ms; };
#if defined(__HIP_DEVICE_COMPILE__)
#define GAML_CALLEE_ARGS(name, set, COV)                                                                                             \
  const unsigned long long name##_u = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(kernargs >> 32)) << 32) |  \
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)kernargs); /* (uniform: scalar loads) */         \
  const __attribute__((address_space(4))) MultiKernArgs* name##_p = (const __attribute__((address_space(4))) MultiKernArgs*)name##_u; \
  const PairedArgs name##_0 = name##_p->a;                                                                                           \
  const PairedArgs name = (set) >= 0 ? with_set<COV>(name##_0, name##_p->ms.set[set]) : name##_0;
#else
#define GAML_CALLEE_ARGS(name, set, COV) const PairedArgs& name = *(const PairedArgs*)nullptr;
#endif
template <bool COV>
__device__ __forceinline__ GenOut compact_general_impl(unsigned long long kernargs, int i, int set) {
  GAML_CALLEE_ARGS(a, set, COV)
  GenOut o{0.0, 0};
  compact_general(a, i, o.add, o.zeros);
  return o;
}
__device__ __noinline__ GenOut compact_general_call(unsigned long long kernargs, int i, int set) { return compact_general_impl<false>(kernargs, i, set); }
__device__ __noinline__ GenOut compact_general_call_cov(unsigned long long kernargs, int i, int set) { return compact_general_impl<true>(kernargs, i, set); }
template <bool COV>
__device__ __forceinline__ GenOut general_pair_impl(unsigned long long kernargs, int i, int dj, int set, int4* lds) {
  GAML_CALLEE_ARGS(a, set, COV)
  GenOut o{0.0, 0};
  int4 priv[2 * kGenCands];
  int4* const cand = lds ? lds : priv;
  const int4 none = make_int4(-1, 0, 0, 0);
  int4 r1[4], r2[4];
  double acc;
  if (dj < 0) {  // a table pair of class 1 / 2: its inline copies
    const bool four = i >= a.n01;
    const size_t at = four ? (size_t)2 * (a.n01 - a.n0) + (size_t)4 * (i - a.n01) : (size_t)2 * (i - a.n0);
#pragma unroll
    for (int k = 0; k < 4; k++) { const bool has = four || k < 2; r1[k] = has ? a.inl[0][at + (has ? k : 0)] : none; r2[k] = has ? a.inl[1][at + (has ? k : 0)] : none; }
    const uint32_t l12 = a.len12[i - a.n0];
    const int L1 = l12 & 0xffff, L2 = l12 >> 16;
    if (!general_pair_staged<4>(a, r1, r2, L1, L2, acc, cand)) acc = paired_general(a, a.m[0].first[i - a.n0], a.m[1].first[i - a.n0], L1, L2);
    finish_read(a, i, acc, L1, L2, o.add, o.zeros);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { r1[k] = a.dirty_recs[0][4 * (size_t)dj + k]; r2[k] = a.dirty_recs[1][4 * (size_t)dj + k]; }
    const uint32_t l12 = (uint32_t)r1[0].w;
    const int L1 = l12 & 0xffff, L2 = l12 >> 16;
    const int c0 = r2[0].w & 0xff, c1 = (r2[0].w >> 8) & 0xff;
    if (!general_pair_staged<4>(a, r1, r2, L1, L2, acc, cand))
      acc = paired_general_src_masks(a, ListSrc{a.dirty_recs[0] + 4 * (size_t)dj, c0}, ListSrc{a.dirty_recs[1] + 4 * (size_t)dj, c1}, L1, L2);
    finish_read(a, i, acc, L1, L2, o.add, o.zeros);
  }
  return o;
}
__device__ __noinline__ GenOut general_pair_call(unsigned long long kernargs, int i, int dj, int set, int4* lds) { return general_pair_impl<false>(kernargs, i, dj, set, lds); }
__device__ __noinline__ GenOut general_pair_call_cov(unsigned long long kernargs, int i, int dj, int set, int4* lds) { return general_pair_impl<true>(kernargs, i, dj, set, lds); }

// paired_compact4_body with the path sets in the inner loop. acc_s / acc_z: one running sum per (set, thread) in LDS
// (a lane may take several rounds of four pairs; registers cannot be indexed by the set number).
// COV: a launch of penalised sets -- a pair whose term clears the threshold marks both its ends in THIS set's bitmap, where
// paired_compact4_body<.., COV> marks them in the call's.
template <bool GEN, bool ONE, bool COV = false>
__device__ __forceinline__ void paired_compact4_multi_body(const PairedArgs& a, const MultiSets& ms, const SlotRange rg, double* acc_s, int* acc_z, const double* tf) {
  const unsigned stride = (unsigned)rg.blocks * kBlock, n0 = (unsigned)rg.hi;  // (n0: end of this part's slots)
  const char* const rec0 = (const char*)a.rec8[0];
  const char* const rec1 = (const char*)a.rec8[1];
  const char* const memo = (const char*)a.memo;
  char* const probs = (char*)a.probs;
  const uint32_t l12_one = ONE ? a.len_combo[0] : 0u;
  const double logfloor_one = ONE ? a.logfloor_c[0] : 0.0;
  const double covthr_one = COV && ONE ? a.covthr0 : 0.0;
  for (unsigned base = (unsigned)rg.lo + (unsigned)rg.lb * kBlock + threadIdx.x; base < n0; base += 4 * stride) {
    uint2 r1[4], r2[4];
    unsigned lc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // the records: ONCE for all sets
      const unsigned ic = base + k * stride < n0 ? base + k * stride : base;
      r1[k] = *(const uint2*)(rec0 + ic * 8u); r2[k] = *(const uint2*)(rec1 + ic * 8u); lc[k] = ONE ? 0u : (unsigned)a.len_code[ic];
    }
    // (Every set resolves every pair here. Finishing a pair from its set-0 result where no window of it changed -- as the
    // other classes do -- does not pay in this class: the launch lasts as long as its slowest wavefront, and some
    // wavefront always holds a pair on a changed window; the bookkeeping only costs registers. Measured: 26.1 us for
    // four sets this way, 28.7 us with the capture, tools/batch_ablate.py.)
#pragma unroll 1
    for (int s = 0; s < ms.n; s++) {
      const SetDev& sd = ms.set[s];
      const char* const occ0 = (const char*)sd.occ12[0];
      const char* const occ1 = (const char*)sd.occ12[1];
      const double* const tfs = tf ? tf + s * kTfCodes : sd.tfloor_c;  // this set's thresholds per length code (LDS copy when it fits)
      const double log2T = sd.log_two_T, tfloor_one = ONE ? tfs[0] : 0.0;
      const bool last_set = s == ms.n - 1;  // per-read probabilities: those of the last set, as after a sequence of calls
      uint2 o1[4], o2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const Occ12* e1 = (const Occ12*)(occ0 + (r1[k].y != ~0u ? (r1[k].x & 0xffffffu) : 0u) * 12u);
        const Occ12* e2 = (const Occ12*)(occ1 + (r2[k].y != ~0u ? (r2[k].x & 0xffffffu) : 0u) * 12u);
        o1[k] = make_uint2(e1->lo, e1->hi); o2[k] = make_uint2(e2->lo, e2->hi);
      }
      int state[4];
      unsigned skip_bits = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        bool skip;
        state[k] = compact_state(a, r1[k], r2[k], o1[k], o2[k], lc[k], ONE ? l12_one : a.len_combo[lc[k]], base + k * stride < n0, skip);
        skip_bits |= (unsigned)skip << k;
      }
      double2 m[4];
#pragma unroll
      for (int k = 0; k < 4; k++) m[k] = *(const double2*)(memo + (unsigned)max(state[k], 0) * 16u);
      double lsum = 0.0;
      int zeros = 0;
      bool other = false;
      unsigned mark_bits = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        double* const out = (double*)(probs + (base + k * stride) * 8u);
        if (state[k] >= 0) {
          if (COV) mark_bits |= (unsigned)(m[k].x > (ONE ? covthr_one : a.covthr_c[lc[k]])) << k;
          if (last_set) __builtin_nontemporal_store(m[k].x, out);
          const bool floored = m[k].x < (ONE ? tfloor_one : tfs[lc[k]]);
          lsum += floored ? (ONE ? logfloor_one : a.logfloor_c[lc[k]]) : m[k].y - log2T;
          zeros += (int)floored;
        } else if (state[k] > kPairOther) {
          if (last_set) __builtin_nontemporal_store(0.0, out);
          zeros++;
          lsum += ONE ? logfloor_one : a.logfloor_c[kPairZero - state[k]];
        } else other |= state[k] == kPairOther && !((skip_bits >> k) & 1u);
      }
      if (COV) {  // behind the set's sums and stores, as in the single-set body
#pragma unroll
        for (int k = 0; k < 4; k++)
          if ((mark_bits >> k) & 1u) cover_marks_set(sd.cov_bits, sd.slot_base, r1[k], r2[k], o1[k], o2[k]);
      }
      if (__any(other)) {  // scores, but outside the memo: from the tables (rare)
        const PairedArgs b = with_set<COV>(a, sd, tf ? tfs : nullptr);
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
          if (state[k] != kPairOther || ((skip_bits >> k) & 1u)) continue;
          const int i = (int)(base + k * stride);
          Compact1 d;
          compact_load(b, i, true, d);
          d.o1 = d.r1 != kNone8 ? occ8_of(b.occ12[0], (unsigned)(d.r1 & 0xffffff)) : kNone8;
          d.o2 = d.r2 != kNone8 ? occ8_of(b.occ12[1], (unsigned)(d.r2 & 0xffffff)) : kNone8;
          const uint32_t l = b.len_combo[d.lc];
          d.L1 = l & 0xffff; d.L2 = l >> 16;
          CompactPrep q;
          compact_prep(b, d, q);
          compact_finish(b, i, d, q, make_double2(0.0, 0.0), lsum, zeros);
        }
      }
      if (GEN && __any(skip_bits != 0)) {  // as paired_compact4_body
#pragma unroll 1
        for (int k = 0; k < 4; k++)
          if ((skip_bits >> k) & 1u) compact_general_add<COV>((int)(base + k * stride), s, lsum, zeros);
      }
      acc_s[s * kBlock + threadIdx.x] += lsum;
      acc_z[s * kBlock + threadIdx.x] += zeros;
    }
  }
}

// paired_static4_body with the path sets in the inner loop: the static pairs' records AND values come in once for all sets
// (the per-set arithmetic above goes records -> occurrence entries -> memo index -> memo entry, two dependent trips per set;
// here a set costs one: its occurrence entries). Lanes, pairs, the values added and their order are the single-set
// kernel's: a batch gives bit for bit what the sets give one by one.
template <bool GEN, bool ONE, bool COV = false>
__device__ __forceinline__ void paired_static4_multi_body(const PairedArgs& a, const MultiSets& ms, const SlotRange rg, double* acc_s, int* acc_z, const double* tf) {
  const unsigned stride = (unsigned)rg.blocks * kBlock, n0 = (unsigned)rg.hi;
  const char* const rec0 = (const char*)a.rec8[0];
  const char* const rec1 = (const char*)a.rec8[1];
  const char* const sval = (const char*)a.static_val;
  char* const probs = (char*)a.probs;
  const double logfloor_one = ONE ? a.logfloor_c[0] : 0.0;
  const double covthr_one = COV && ONE ? a.covthr0 : 0.0;
  for (unsigned base = (unsigned)rg.lo + (unsigned)rg.lb * kBlock + threadIdx.x; base < n0; base += 4 * stride) {
    uint2 r1[4], r2[4];
    double2 m[4];
    unsigned lc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // records and values: ONCE for all sets
      const unsigned ic = base + k * stride < n0 ? base + k * stride : base;
      r1[k] = *(const uint2*)(rec0 + ic * 8u); r2[k] = *(const uint2*)(rec1 + ic * 8u); m[k] = *(const double2*)(sval + ic * 16u);
      lc[k] = ONE ? 0u : (unsigned)a.len_code[ic];
    }
#pragma unroll 1
    for (int s = 0; s < ms.n; s++) {
      const SetDev& sd = ms.set[s];
      const char* const occ0 = (const char*)sd.occ12[0];
      const char* const occ1 = (const char*)sd.occ12[1];
      const double* const tfs = tf ? tf + s * kTfCodes : sd.tfloor_c;
      const double log2T = sd.log_two_T, tfloor_one = ONE ? tfs[0] : 0.0;
      const bool last_set = s == ms.n - 1;
      uint2 o1[4], o2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const unsigned w1 = (r1[k].x & 0xffffffu) & (0u - (unsigned)(r1[k].y != ~0u)), w2 = (r2[k].x & 0xffffffu) & (0u - (unsigned)(r2[k].y != ~0u));
        const Occ12* e1 = (const Occ12*)(occ0 + w1 * 12u);
        const Occ12* e2 = (const Occ12*)(occ1 + w2 * 12u);
        o1[k] = make_uint2(e1->lo, e1->hi); o2[k] = make_uint2(e2->lo, e2->hi);
      }
      double lsum = acc_s[s * kBlock + threadIdx.x];  // (the running sum of this lane and set: additions in the single-set kernel's order)
      int zeros = acc_z[s * kBlock + threadIdx.x];
      unsigned skip_bits = 0, mark_bits = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {  // as paired_static4_body, statement for statement
        const bool none1 = r1[k].y == ~0u, none2 = r2[k].y == ~0u;
        const bool here = (base + k * stride < n0) & !(none1 & (r1[k].x == 0xfffffffeu));
        const bool w1 = !none1 & (o1[k].y != ~0u), w2 = !none2 & (o2[k].y != ~0u);
        const bool gen = here & ((w1 & ((int)o1[k].y < 0)) | (w2 & ((int)o2[k].y < 0)));
        const bool same = (o1[k].x == o2[k].x) & (((o1[k].y ^ o2[k].y) >> 16) == 0);
        const int p1 = (int)(__funnelshift_r(r1[k].x, r1[k].y, 24) & 0xfffffffu), p2 = (int)(__funnelshift_r(r2[k].x, r2[k].y, 24) & 0xfffffffu);
        const bool kept = (p1 >= (int)(short)(o1[k].y & 0xffffu)) & (p2 >= (int)(short)(o2[k].y & 0xffffu));
        const bool both = here & !gen & w1 & w2;
        const bool scores = both & same & kept;
        const bool poison = both & !same;
        const bool counted = here & !gen;
        skip_bits |= (unsigned)gen << k;
        const double t = scores ? m[k].x : 0.0;
        const bool floored = counted & (!scores | (t < (ONE ? tfloor_one : tfs[lc[k]])));
        const double lf = ONE ? logfloor_one : a.logfloor_c[lc[k]];
        double add = floored ? lf : m[k].y - log2T;
        add = counted ? add : 0.0;
        add = poison ? __builtin_nan("") : add;
        lsum += add;
        zeros += (int)floored;
        if (counted && last_set) __builtin_nontemporal_store(t, (double*)(probs + (base + k * stride) * 8u));
        if (COV) mark_bits |= (unsigned)(scores & (t > (ONE ? covthr_one : a.covthr_c[lc[k]]))) << k;
      }
      if (COV) {  // behind the set's sums and stores, into this set's bitmap
#pragma unroll
        for (int k = 0; k < 4; k++)
          if ((mark_bits >> k) & 1u) cover_marks_set(sd.cov_bits, sd.slot_base, r1[k], r2[k], o1[k], o2[k]);
      }
      if (GEN && __any(skip_bits != 0)) {  // as paired_static4_body
#pragma unroll 1
        for (int k = 0; k < 4; k++)
          if ((skip_bits >> k) & 1u) compact_general_add<COV>((int)(base + k * stride), s, lsum, zeros);
      }
      acc_s[s * kBlock + threadIdx.x] = lsum;
      acc_z[s * kBlock + threadIdx.x] = zeros;
    }
  }
}

// Classes 1 and 2 with the path sets in the inner loop (paired_regs_body's pairs, lane -> pair mapping and order of
// additions): records once, set 0 resolved and captured, later sets finished from the capture unless one of the
// pair's windows changed.
template <int K, bool GEN, bool COV = false>
__device__ __forceinline__ void paired_regs_multi_body(const PairedArgs& a, const MultiSets& ms, int lb, int slot_lo, int slot_hi, int block_lo,
                                                       int block_hi, double* acc_s, int* acc_z, const double* tf) {
  for (int i = slot_lo + (lb - block_lo) * kBlock + threadIdx.x; i < slot_hi; i += (block_hi - block_lo) * kBlock) {
    const uint32_t l12 = a.len12[i - a.n0];
    const size_t at = K == 2 ? (size_t)2 * (i - a.n0) : (size_t)2 * (a.n01 - a.n0) + (size_t)4 * (i - a.n01);
    int4 r1[K], r2[K];
#pragma unroll
    for (int k = 0; k < K; k++) { r1[k] = a.inl[0][at + k]; r2[k] = a.inl[1][at + k]; }
    const bool dirty = r1[0].x == kDirtyWid;  // scored from the delta lists
    unsigned chg = ms.chg[0] ? 0u : 0xffu;
    if (ms.chg[0] && !dirty) {
#pragma unroll
      for (int k = 0; k < K; k++) chg |= (r1[k].x >= 0 ? ms.chg[0][r1[k].x] : 0u) | (r2[k].x >= 0 ? ms.chg[1][r2[k].x] : 0u);
    }
    PairVal val{0.0, 0.0, 0, 0};
    bool general = false;
#pragma unroll 1
    for (int s = 0; s < ms.n; s++) {
      const PairedArgs b = with_set<COV>(a, ms.set[s], tf ? tf + s * kTfCodes : nullptr);
      double lsum = acc_s[s * kBlock + threadIdx.x];
      int zeros = acc_z[s * kBlock + threadIdx.x];
      if (s == 0 || ((chg >> s) & 1u)) {
        RegCands<K> x, y;
        const bool m1 = cands_from_records<K>(b.m[0], r1, x), m2 = cands_from_records<K>(b.m[1], r2, y);
        general = !dirty && (m1 || m2);  // a window that occurs several times: general_pair_call
        val.kind = 0;
        if (!dirty && !general) score_cands_and_finish<K>(b, i, l12, x, y, lsum, zeros, &val);
      } else {
        finish_val(b, i, val, s == ms.n - 1, lsum, zeros);
      }
      if (GEN && general) general_pair_add<COV>(i, -1, s, nullptr, lsum, zeros);  // (in every set: val holds nothing of such a pair)
      acc_s[s * kBlock + threadIdx.x] = lsum;
      acc_z[s * kBlock + threadIdx.x] = zeros;
    }
  }
}

// paired_delta_body with the path sets in the inner loop
template <bool GEN, bool COV = false>
__device__ __forceinline__ void paired_delta_multi_body(const PairedArgs& a, const MultiSets& ms, int db, int delta_blocks, double* acc_s, int* acc_z, const double* tf) {
  for (int dj = db * kBlock + threadIdx.x; dj < a.dstate[kDsDirty]; dj += delta_blocks * kBlock) {
    const int i = a.dirty_slots[dj];
    const int sp = a.dirty_spill[dj];
    const bool mine = sp < 0;  // (sp >= 0, a long list: one WAVE scores it. Such a lane stays in the loop: the note words are
                               // written by the wave's lane 0 from a ballot over ALL its lanes)
    int4 r0[4], r1[4];
    int c0 = 0, c1 = 0;
    unsigned chg = ms.chg[0] ? 0u : 0xffu;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      r0[k] = a.dirty_recs[0][4 * (size_t)dj + k];
      r1[k] = a.dirty_recs[1][4 * (size_t)dj + k];
      c0 += r0[k].x >= 0; c1 += r1[k].x >= 0;
      if (ms.chg[0]) chg |= (r0[k].x >= 0 ? ms.chg[0][r0[k].x] : 0u) | (r1[k].x >= 0 ? ms.chg[1][r1[k].x] : 0u);
    }
    const uint32_t l12 = (uint32_t)r0[0].w;  // the pair's read lengths travel with its first record (paired_upload_delta)
    PairVal val{0.0, 0.0, 0, 0};
    bool general = false;  // as resolved last: a set whose tables agree with its predecessor's on this pair's windows inherits it
#pragma unroll 1
    for (int s = 0; s < ms.n; s++) {
      const PairedArgs b = with_set<COV>(a, ms.set[s], tf ? tf + s * kTfCodes : nullptr);
      double lsum = acc_s[s * kBlock + threadIdx.x];
      int zeros = acc_z[s * kBlock + threadIdx.x];
      if (!mine) {
      } else if (s == 0 || ((chg >> s) & 1u)) {
        RegCands<4> x, y;
        const bool m0 = cands_from_records<4>(b.m[0], r0, x), m1 = cands_from_records<4>(b.m[1], r1, y);
        general = m0 || m1;  // a window that occurs several times in this path set: general_pair_call (as paired_delta_body)
        val.kind = 0;
        if (!general) score_cands_and_finish<4>(b, i, l12, x, y, lsum, zeros, &val);
        else if (!GEN) lsum += __builtin_nan("");  // cannot happen (a launch without notes has no such window): poisoned, reported by combine()
      } else {
        finish_val(b, i, val, s == ms.n - 1, lsum, zeros);
      }
      if (GEN && mine && general) general_pair_add<COV>(i, dj, s, nullptr, lsum, zeros);
      acc_s[s * kBlock + threadIdx.x] = lsum;
      acc_z[s * kBlock + threadIdx.x] = zeros;
    }
  }
}

// the sets (bits) in which one of a pair's windows changed, over all its records of one mate: lanes stride, wave OR
template <class Src>
__device__ __forceinline__ unsigned wave_changed(const Src& src, const unsigned char* chg, int lane) {
  unsigned m = 0;
  const int cnt = src.count();
  for (int k = lane; k < cnt; k += 64) { const int4 r = src.get(k); if (r.x >= 0) m |= chg[r.x]; }
  for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, 64);
  return m;
}

// paired_overflow_body with the path sets in the inner loop: wave w keeps its running sums per set in acc (lane 0's)
template <bool COV = false>
__device__ __forceinline__ void paired_overflow_multi_body(const PairedArgs& a, const MultiSets& ms, int ovf_block, int ovf_blocks,
                                                           int4 (*cand)[2][kOvfCap], double* acc_s, int* acc_z, const double* tf) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_global = ovf_block * (kBlock / 64) + wave;
  const int n_waves = ovf_blocks * (kBlock / 64);
  const int n_table = a.n - a.n_main;
  const int n_items = n_table + a.dstate[kDsSpill];
  int4* c1 = cand[wave][0];
  int4* c2 = cand[wave][1];
  for (int item = wave_global; item < n_items; item += n_waves) {  // fixed item -> wave assignment
    int i, L1, L2;
    TableSrc t1{&a.m[0], make_int4(-1, 0, 0, 0)}, t2{&a.m[1], make_int4(-1, 0, 0, 0)};
    ListSrc l1{nullptr, 0}, l2{nullptr, 0};
    const bool table = item < n_table;
    if (table) {
      i = a.n_main + item;
      t1.r0 = a.m[0].first[i - a.n0]; t2.r0 = a.m[1].first[i - a.n0];
      const uint32_t l12 = a.len12[i - a.n0];
      if (t1.r0.x == kDirtyWid) continue;  // a class-3 pair that is on the delta list: scored there
      L1 = l12 & 0xffff; L2 = l12 >> 16;
    } else {
      const int sp = item - n_table;
      i = a.spill_slot[sp];
      const uint32_t l12 = i < a.n0 ? a.len_combo[a.len_code[i]] : a.len12[i - a.n0];
      L1 = l12 & 0xffff; L2 = l12 >> 16;
      const int2 g0 = a.spill_rng[0][sp], g1 = a.spill_rng[1][sp];
      l1 = ListSrc{a.spill_recs[0] + g0.x, g0.y};
      l2 = ListSrc{a.spill_recs[1] + g1.x, g1.y};
    }
    unsigned chg = 0xffu;
    if (ms.chg[0]) chg = table ? (wave_changed(t1, ms.chg[0], lane) | wave_changed(t2, ms.chg[1], lane)) : (wave_changed(l1, ms.chg[0], lane) | wave_changed(l2, ms.chg[1], lane));
    PairVal val{0.0, 0.0, 0, 0};
    for (int s = 0; s < ms.n; s++) {
      const PairedArgs b = with_set<COV>(a, ms.set[s], tf ? tf + s * kTfCodes : nullptr);
      double lsum = 0.0;
      int zeros = 0;
      if (s == 0 || ((chg >> s) & 1u)) {  // wave-uniform
        TableSrc u1{&b.m[0], t1.r0}, u2{&b.m[1], t2.r0};
        const double acc = table ? wave_score_pair(b, u1, u2, L1, L2, c1, c2, lane) : wave_score_pair(b, l1, l2, L1, L2, c1, c2, lane);
        if (lane == 0) finish_read(b, i, acc, L1, L2, lsum, zeros, &val);
      } else if (lane == 0) {
        finish_val(b, i, val, s == ms.n - 1, lsum, zeros);
      }
      if (lane == 0) { acc_s[s * (kBlock / 64) + wave] += lsum; acc_z[s * (kBlock / 64) + wave] += zeros; }
    }
  }
}

// COV: every set of the launch has a coverage penalty (the read set has one) and a bitmap of its own (SetDev::cov_bits): class 0
// marks from the memo / streamed-value bodies, everything else through the set's view (with_set<true>). The host runs such a
// launch without the capture (MultiSets::chg null): a pair finished from its set-0 result would still have to mark in set s,
// at positions that depend on set s's layout.
template <bool GEN, bool COV = false>
__global__ __launch_bounds__(kBlock, 5) void paired_score_multi_kernel(PairedArgs a, MultiSets ms) {
  __shared__ double sh_s[kBlock / 64];
  __shared__ int sh_z[kBlock / 64];
  // the lane-per-pair blocks keep one running sum per (set, thread) here (8 sets x 256 threads x (8 + 4) B = 24 KB);
  // the wave-per-pair blocks stage candidates here (16 KB) and keep one running sum per (set, wave) behind them:
  // block-uniform roles, one buffer
  __shared__ __align__(16) unsigned char sh_raw[kMaxSets * kBlock * 12];
  constexpr size_t kCandBytes = sizeof(int4) * (kBlock / 64) * 2 * kOvfCap;
  static_assert(kCandBytes + kMaxSets * (kBlock / 64) * 12 <= sizeof(sh_raw), "candidate staging + per-wave sums must fit");
  const int lb = a.total_blocks - 1 - (int)blockIdx.x;
  // every set's thresholds per length code: read once per block (they sit in host-written device memory, a round trip
  // each), not once per set and pair
  __shared__ double sh_tf[kMaxSets * kTfCodes];
  const double* tf = a.n_codes <= kTfCodes ? sh_tf : nullptr;
  if (tf && threadIdx.x < kMaxSets * kTfCodes) {
    const int s = threadIdx.x / kTfCodes, k = threadIdx.x % kTfCodes;
    sh_tf[threadIdx.x] = s < ms.n && k < a.n_codes ? ms.set[s].tfloor_c[k] : 0.0;
  }
  if (lb < a.main_blocks) {
    double* acc_s = (double*)sh_raw;
    int* acc_z = (int*)(sh_raw + kMaxSets * kBlock * 8);
    for (int s = 0; s < ms.n; s++) { acc_s[s * kBlock + threadIdx.x] = 0.0; acc_z[s * kBlock + threadIdx.x] = 0; }
    __syncthreads();
    const int cls = lb < a.blocks0 ? 0 : lb < a.blocks01 ? 1 : lb < a.blocks012 ? 2 : 3;
    if ((ms.skip_classes >> cls) & 1) {  // a class of blocks left out (bit per class; set by the warm-up launch only, for bit 4 below)
      if (threadIdx.x == 0) for (int s = 0; s < ms.n; s++) { ms.set[s].part_sum[lb] = 0.0; ms.set[s].part_zero[lb] = 0; }
      return;
    }
    if (lb < a.blocks0) {
      // (both parts of class 0 resolve every pair per set here: the lanes, pairs and order of additions are the single-set
      // kernel's, and so are the values -- a static memo index is the index the per-call arithmetic arrives at)
      const SlotRange rg = compact_range(a, lb);
      // the static part streams its values like the single-set kernel (same condition as there: memo present, no coverage marks)
      // (a penalised launch keeps streaming, as paired_score_kernel<.., COV> does)
      const bool stat = lb < a.blocks0a && a.memo && (COV || !a.cov_bits) && a.static_val;
      if (a.n_codes == 1) {
        if (stat) paired_static4_multi_body<GEN, true, COV>(a, ms, rg, acc_s, acc_z, tf);
        else paired_compact4_multi_body<GEN, true, COV>(a, ms, rg, acc_s, acc_z, tf);
      } else {
        __shared__ uint32_t sh_combo[256];
        __shared__ double sh_logfloor[256];
        for (int k = threadIdx.x; k < a.n_codes; k += kBlock) { sh_combo[k] = a.len_combo[k]; sh_logfloor[k] = a.logfloor_c[k]; }
        const double* covthr_lds = nullptr;
        if constexpr (COV) {  // the coverage thresholds per length code (per read set, not per path set): looked up once per pair and set
          __shared__ double sh_covthr[256];
          for (int k = threadIdx.x; k < a.n_codes; k += kBlock) sh_covthr[k] = a.covthr_c[k];
          covthr_lds = sh_covthr;
        }
        __syncthreads();
        PairedArgs b = a;
        b.len_combo = sh_combo; b.logfloor_c = sh_logfloor;
        if (COV) b.covthr_c = covthr_lds;
        if (stat) paired_static4_multi_body<GEN, false, COV>(b, ms, rg, acc_s, acc_z, tf);
        else paired_compact4_multi_body<GEN, false, COV>(b, ms, rg, acc_s, acc_z, tf);
      }
    } else if (lb < a.blocks01) paired_regs_multi_body<2, GEN, COV>(a, ms, lb, a.n0, a.n01, a.blocks0, a.blocks01, acc_s, acc_z, tf);
    else if (lb < a.blocks012) paired_regs_multi_body<4, GEN, COV>(a, ms, lb, a.n01, a.n_main, a.blocks01, a.blocks012, acc_s, acc_z, tf);
    else paired_delta_multi_body<GEN, COV>(a, ms, lb - a.blocks012, a.main_blocks - a.blocks012, acc_s, acc_z, tf);
    for (int s = 0; s < ms.n; s++) {
      double lsum = acc_s[s * kBlock + threadIdx.x];
      int zeros = acc_z[s * kBlock + threadIdx.x];
      block_reduce(lsum, zeros, sh_s, sh_z);
      if (threadIdx.x == 0) { ms.set[s].part_sum[lb] = lsum; ms.set[s].part_zero[lb] = zeros; }
      __syncthreads();  // sh_s / sh_z are reused by the next set
    }
    return;
  }
  if ((ms.skip_classes >> 4) & 1) {
    if (threadIdx.x == 0) for (int s = 0; s < ms.n; s++) { ms.set[s].part_sum[lb] = 0.0; ms.set[s].part_zero[lb] = 0; }
    return;
  }
  double* acc_s = (double*)(sh_raw + kCandBytes);
  int* acc_z = (int*)(sh_raw + kCandBytes + kMaxSets * (kBlock / 64) * 8);
  if (threadIdx.x < kMaxSets * (kBlock / 64)) { acc_s[threadIdx.x] = 0.0; acc_z[threadIdx.x] = 0; }
  __syncthreads();
  paired_overflow_multi_body<COV>(a, ms, lb - a.main_blocks, a.total_blocks - a.main_blocks, (int4(*)[2][kOvfCap])sh_raw, acc_s, acc_z, tf);
  __syncthreads();
  for (int s = 0; s < ms.n; s++) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double lsum = lane == 0 ? acc_s[s * (kBlock / 64) + wave] : 0.0;
    int zeros = lane == 0 ? acc_z[s * (kBlock / 64) + wave] : 0;
    block_reduce(lsum, zeros, sh_s, sh_z);
    if (threadIdx.x == 0) { ms.set[s].part_sum[lb] = lsum; ms.set[s].part_zero[lb] = zeros; }
    __syncthreads();
  }
}

}  // namespace gaml
