// pps_map_window.h -- what the kernels that walk a built map share (pps_map.hip: k_map_build, k_map_build_posed; pps_grid.hip: the grid
// passes over the same indices): the chunk window of a workgroup, the search in an offset table, and the small wave and workgroup
// reductions of the map's compactions.
//
// The window.  A workgroup owns 256 consecutive points of the built map.  Thread 0 looks up the chunk of the first point in the offset
// table (binary search in global memory) and the workgroup stages the next 256 chunks in LDS: chunks in the table are non-empty, so the
// 256 points end inside that window; each thread then searches the window.
#pragma once
#include "pps_map.h"

namespace pps {

// bits of the wave mask m below the calling lane
__device__ __forceinline__ int map_lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
}

// the row lo of an ascending offset table with off[lo] <= i < off[lo + 1], among rows 0 .. n-1 (off[0] <= i; off[n] is not read)
__device__ __forceinline__ int map_find(const long long* off, int n, long long i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// AUX: the window carries a fourth row of int per chunk (posed build: the frame's row in the motion table; grid: the landmark's row)
template <bool AUX> struct MapWindowAux { int aux[kMapThreads]; };
template <> struct MapWindowAux<false> {};
template <bool AUX>
struct MapWindow : MapWindowAux<AUX> {
  long long off[kMapThreads + 1], src[kMapThreads];
  int slot[kMapThreads];
  int c0;                                      // the table row of window row 0
};

// every thread of the workgroup calls it; first: the workgroup's first point.  Behind it the window is complete for all of them.
template <bool AUX>
__device__ __forceinline__ void map_stage_window(MapWindow<AUX>& w, const long long* out_off, const long long* src_off, const int* slot, const int* aux,
                                                 int n_sel, long long first) {
  const int tid = threadIdx.x;
  if (tid == 0) w.c0 = map_find(out_off, n_sel, first);
  __syncthreads();
  const int c0 = w.c0;
  for (int j = tid; j <= kMapThreads; j += kMapThreads) w.off[j] = c0 + j <= n_sel ? out_off[c0 + j] : 0x7fffffffffffffffLL;
  if (c0 + tid < n_sel) {
    w.src[tid] = src_off[c0 + tid]; w.slot[tid] = slot[c0 + tid];
    if constexpr (AUX) w.aux[tid] = aux[c0 + tid];
  }
  __syncthreads();
}

// the window row of point i of the workgroup
template <bool AUX>
__device__ __forceinline__ int map_window_find(const MapWindow<AUX>& w, long long i) { return map_find(w.off, kMapThreads, i); }

// Workgroups of kMapThreads; s: one T per thread in LDS.  map_block_scan: the inclusive prefix of v over the threads (the last thread's is
// the sum); map_block_sum: the sum of v, valid in thread 0.
template <class T>
__device__ __forceinline__ T map_block_scan(T* s, T v) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kMapThreads; d <<= 1) {
    const T u = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += u;
    __syncthreads();
  }
  return s[tid];
}
template <class T>
__device__ __forceinline__ T map_block_sum(T* s, T v) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = kMapThreads / 2; d > 0; d >>= 1) {
    if (tid < d) s[tid] += s[tid + d];
    __syncthreads();
  }
  return s[0];
}

}  // namespace pps
