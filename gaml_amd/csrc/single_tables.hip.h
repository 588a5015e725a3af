// single_tables.hip.h -- the read-major record table of a single-end set, built ON THE DEVICE from a byte mirror of the
// host's record pool (the device counterpart of build_read_major, host_model.cc; taken only where the context says so:
// gaml_hip_set_single_device, off by default).
//
//   pool      int4 view of gaml_aligment {position, edit distance, read, orientation}: ShortMate::pool as it stands on the
//             host, append-only in filing order; a window's records are contiguous, ordered by (position, read)
//   hdr       one StWin per ACTIVE window with records, ascending window id: where its records sit in the pool, how many,
//             and how many records the windows before it hold (the host writes these few thousand headers per build)
//
// One build = a chain of dispatches on the evaluation's stream, no host round trip in between:
//   st_clear_kernel   first[r] = {-1, 0, 0, 0} for every read (a byte memset cannot write that pattern)
//   st_keys_kernel    a lane per record of the active windows, numbered g in (window id, pool order): key = its read,
//                     payload = g
//   rs_sort           stable over ceil(log2(reads)) bits: a read's records end up contiguous and keep the (window id, pool
//                     order) sequence -- the order build_read_major visits them in, which single_read_acc's (record,
//                     occurrence) order depends on
//   st_heads_kernel   flag[p] = 1 where a read's run starts
//   tb_scan_*         E(p) = flags before p (exclusive prefix; H(p) = E(p) + flag[p] is the inclusive one)
//   st_fill_kernel    a lane per sorted position p of a run that starts at b and holds L records:
//                       head (p == b)  first[read] = record, flags |= (L - 1) << 9, link = b - E(b)  [= b + 1 - H(b)]
//                       other          extra[p - E(p)] = record                                     [= p - H(p)]
//                     b - E(b) counts the records before b that are not heads = the sum of (count - 1) over the reads before
//                     this one = build_read_major's start[]; inside the run E(p) = E(b) + 1, so p - E(p) = start + (p - b) - 1
//                     = start[] + seen[] - 1; L - 1 = cnt[] - 1.
// No atomics, no order that depends on scheduling: two builds of one state give equal bytes (the development build checks
// them against build_read_major: gaml_hip_debug_single_table_check).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "radix_sort.hip.h"

namespace gaml {

struct StWin { int first, count, wid, before; };  // 16 bytes: one load

// the last header whose `before` <= g (headers hold at least one record each, so `before` strictly increases)
__device__ __forceinline__ int4 st_window_of(const int4* hdr, int n_hdr, int g) {
  int lo = 0, hi = n_hdr - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (hdr[mid].w <= g) lo = mid; else hi = mid - 1; }
  return hdr[lo];
}

__global__ __launch_bounds__(256) void st_clear_kernel(int4* first, int n_reads) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n_reads; r += gridDim.x * 256) first[r] = make_int4(-1, 0, 0, 0);
}

__global__ __launch_bounds__(256) void st_keys_kernel(const int4* pool, const int4* hdr, int n_hdr, int total, rs_u64* keys, unsigned* vals) {
  for (int g = blockIdx.x * 256 + threadIdx.x; g < total; g += gridDim.x * 256) {
    const int4 w = st_window_of(hdr, n_hdr, g);
    const int4 r = pool[w.x + (g - w.w)];
    keys[g] = (rs_u64)(unsigned)r.z;
    vals[g] = (unsigned)g;
  }
}

__global__ __launch_bounds__(256) void st_heads_kernel(const rs_u64* keys, int total, int* flag) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) flag[p] = (p == 0 || keys[p - 1] != keys[p]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void st_fill_kernel(const int4* pool, const int4* hdr, int n_hdr, const rs_u64* keys, const unsigned* vals, const int* flag,
                                                      const int* before, int total, int n_reads, int4* first, int4* extra) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
    const rs_u64 key = keys[p];
    const int g = (int)vals[p];
    const int4 w = st_window_of(hdr, n_hdr, g);
    const int4 r = pool[w.x + (g - w.w)];
    int4 q = make_int4(w.z, r.x, (r.y & 0xff) | ((r.w & 1) << 8), 0);
    const int at = p - before[p];
    if (flag[p]) {
      int lo = p + 1, hi = total;  // the run's end: the first position behind p with another key (keys ascend)
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] == key) lo = mid + 1; else hi = mid; }
      q.z |= (lo - p - 1) << 9;
      q.w = at;
      if (key < (rs_u64)n_reads) first[key] = q;
    } else {
      extra[at] = q;  // (at <= p < total: the table holds `total` entries)
    }
  }
}

}  // namespace gaml
