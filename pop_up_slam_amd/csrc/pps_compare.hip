// pps_compare.hip -- a pop-up frame against the rendered map view (include/pps.h: pps_map_compare).
//
//   k_compare          one thread per pixel and pass; a workgroup of 256 owns kComparePasses x 256 consecutive pixels of the raster.  A pixel
//                      reads 24 B: the 16-byte pop-up point, the pop-up plane id and the render's PLANE ID (not its cell: 4 B against 8, and
//                      either way the row is one binary search away -- in the ascending node ids of the plane table here).  Its table entry
//                      (frame plane, row; the margins are entries like any other) is its key.  The lanes of a wave that share a key find
//                      each other with a ballot on the key of the first lane that is left, as the partition kernels of pps_map.hip do for
//                      planes: n and n_agree are population counts of ballots, sum_q and sum_q2 are summed over the matching lanes with
//                      xor shuffles of 32-bit pieces (|q| <= 2^19; q^2 goes as its low 20 bits and the rest, 64 of either fit an int).  The
//                      loop over distinct keys takes at most 64 turns.  The wave's leader of a key adds the four sums to the workgroup's
//                      table in LDS: kCompareSlots entries, open addressing, a slot claimed with a compare-and-swap on its key, at most
//                      kCompareProbes slots tried.  A key that finds no slot goes to memory from that wave directly.  Behind one barrier
//                      the workgroup adds every slot it filled to the table in memory: one set of vector atomic adds per distinct entry
//                      it saw.  No workgroup waits for another; every accumulator is an integer, so the order of the adds does not show.
//   k_compare_scan     one workgroup per table row (frame planes, then the row "no frame"): the best landmark of the plane by the stated
//                      order, its margins, the number of its entries with n >= 1.
//   k_compare_emit     one workgroup per frame plane writes its pairs behind those of the planes before it (an exclusive prefix over at most
//                      65 counts, summed by every thread; inside the plane the compaction of k_render_slots); one more workgroup writes
//                      the per-row records and the totals.
//
// Compiled without contraction (Makefile), like every file that includes pps_grid_cell.h.
#include <hip/hip_runtime.h>

#include <climits>

#include "pps_compare.h"
#include "pps_map_window.h"

namespace pps {
namespace {

// the row of the plane table with node id `id`, n_rows if there is none
__device__ __forceinline__ int compare_find_row(const int* __restrict__ ids, int n_rows, int id) {
  int lo = 0, hi = n_rows;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < n_rows && ids[lo] == id) ? lo : n_rows;
}

// the sums v of table entry `key`, from one lane of a wave: into the workgroup's table if a slot can be had, else to memory
__device__ __forceinline__ void compare_add(int* s_key, unsigned long long (*s_val)[4], unsigned long long* table, int key,
                                            const unsigned long long v[4]) {
  unsigned int h = ((unsigned int)key * 2654435761u) >> (32 - kCompareSlotBits);
  for (int p = 0; p < kCompareProbes; p++) {
    const int old = atomicCAS(&s_key[h], -1, key);
    if (old == -1 || old == key) {
      for (int j = 0; j < 4; j++)
        if (v[j]) atomicAdd(&s_val[h][j], v[j]);
      return;
    }
    h = (h + 1u) & (unsigned int)(kCompareSlots - 1);
  }
  for (int j = 0; j < 4; j++)
    if (v[j]) atomicAdd(&table[4 * (size_t)key + j], v[j]);
}

__global__ __launch_bounds__(kMapThreads) void k_compare(CompareArgs a) {
  __shared__ int s_key[kCompareSlots];
  __shared__ unsigned long long s_val[kCompareSlots][4];
  __shared__ unsigned long long s_bad;
  const int tid = threadIdx.x, lane = tid & 63;
  const int cols = a.n_rows + 1;
  for (int i = tid; i < kCompareSlots; i += kMapThreads) {
    s_key[i] = -1;
    for (int j = 0; j < 4; j++) s_val[i][j] = 0ull;
  }
  if (tid == 0) s_bad = 0ull;
  __syncthreads();
  const long long first = (long long)blockIdx.x * (kComparePasses * kMapThreads) + tid;
  MapPt pt[kComparePasses];
  int kf[kComparePasses], vid[kComparePasses];
#pragma unroll
  for (int it = 0; it < kComparePasses; it++) {                    // the loads of all passes first: they do not wait for each other
    const long long px = first + (long long)it * kMapThreads;
    pt[it] = MapPt{0.f, 0.f, 0.f, 0u}; kf[it] = -1; vid[it] = -1;
    if (px < a.npx) {
      pt[it] = a.cloud[px]; kf[it] = a.frame_id[px];
      if (a.view_id) vid[it] = a.view_id[px];
    }
  }
  int n_bad = 0;                                                   // (wave-uniform)
#pragma unroll
  for (int it = 0; it < kComparePasses; it++) {
    const long long px = first + (long long)it * kMapThreads;
    int key = -1;
    bool agree = false, bad = false;
    long long q = 0;
    if (px < a.npx) {
      int k = a.nplanes;
      if (kf[it] >= 0 && kf[it] < a.nplanes) { if ((pt[it].rgba >> 24) & 1u) k = kf[it]; }
      else if (kf[it] != -1) bad = true;
      const int r = vid[it] == -1 ? a.n_rows : compare_find_row(a.ids, a.n_rows, vid[it]);
      key = k * cols + r;
      if (k < a.nplanes && r < a.n_rows) {
        const ComparePlane c = a.planes[r];
        double e;
        agree = compare_point(c, pt[it].x, pt[it].y, pt[it].z, a.tol, &e, &q);
      }
    }
    n_bad += __popcll(__ballot(bad));
    unsigned long long rem = __ballot(key >= 0);
    while (rem) {                                                  // one turn per distinct entry among the 64 pixels (wave-uniform)
      const int leader = __ffsll((long long)rem) - 1;
      const int kk = __builtin_amdgcn_readlane(key, leader);
      const bool mine = key == kk;
      const unsigned long long m = __ballot(mine);
      unsigned long long v[4] = {(unsigned long long)__popcll(m), 0ull, 0ull, 0ull};
      if (kk / cols < a.nplanes && kk % cols < a.n_rows) {         // a pair: the margins carry no distance
        v[1] = (unsigned long long)__popcll(__ballot(mine && agree));
        const long long q2 = mine ? q * q : 0;
        int sq = mine ? (int)q : 0, lo = (int)(q2 & 0xfffff), hi = (int)(q2 >> 20);
        for (int d = 1; d < 64; d <<= 1) { sq += __shfl_xor(sq, d); lo += __shfl_xor(lo, d); hi += __shfl_xor(hi, d); }
        v[2] = (unsigned long long)(long long)sq;
        v[3] = ((unsigned long long)hi << 20) + (unsigned long long)lo;
      }
      if (lane == leader) compare_add(s_key, s_val, a.table, kk, v);
      rem &= ~m;
    }
  }
  if (lane == 0 && n_bad) atomicAdd(&s_bad, (unsigned long long)n_bad);
  __syncthreads();
  if (tid < kCompareSlots) {
    const int key = s_key[tid];
    if (key >= 0)
      for (int j = 0; j < 4; j++) {
        const unsigned long long v = s_val[tid][j];
        if (v) atomicAdd(&a.table[4 * (size_t)key + j], v);
      }
  }
  if (tid == kCompareSlots && s_bad) atomicAdd(&a.table[4 * compare_entries(a.nplanes, a.n_rows)], s_bad);
}

// (agree, n, row) of a candidate: more agree wins, then more n, then the earlier row
__device__ __forceinline__ bool compare_better(unsigned long long a1, unsigned long long n1, int r1, unsigned long long a2, unsigned long long n2, int r2) {
  return a1 > a2 || (a1 == a2 && (n1 > n2 || (n1 == n2 && r1 < r2)));
}

__global__ __launch_bounds__(kMapThreads) void k_compare_scan(CompareFinishArgs a) {
  __shared__ unsigned long long s_sum[kMapThreads], s_ba[kMapThreads], s_bn[kMapThreads];
  __shared__ int s_cnt[kMapThreads], s_br[kMapThreads];
  const int tid = threadIdx.x, k = blockIdx.x;
  const unsigned long long* row = a.table + 4 * (size_t)k * (size_t)(a.n_rows + 1);
  unsigned long long sum = 0, ba = 0, bn = 0;
  int cnt = 0, br = INT_MAX;
  for (int r = tid; r < a.n_rows; r += kMapThreads) {
    const unsigned long long n = row[4 * (size_t)r], ag = row[4 * (size_t)r + 1];
    sum += n; cnt += n > 0 ? 1 : 0;
    if (ag >= 1 && compare_better(ag, n, r, ba, bn, br)) { ba = ag; bn = n; br = r; }
  }
  s_sum[tid] = sum; s_cnt[tid] = cnt; s_ba[tid] = ba; s_bn[tid] = bn; s_br[tid] = br;
  __syncthreads();
  for (int d = kMapThreads / 2; d > 0; d >>= 1) {
    if (tid < d) {
      s_sum[tid] += s_sum[tid + d]; s_cnt[tid] += s_cnt[tid + d];
      if (compare_better(s_ba[tid + d], s_bn[tid + d], s_br[tid + d], s_ba[tid], s_bn[tid], s_br[tid])) {
        s_ba[tid] = s_ba[tid + d]; s_bn[tid] = s_bn[tid + d]; s_br[tid] = s_br[tid + d];
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  a.block->pair_cnt[k] = k < a.nplanes ? (long long)s_cnt[0] : 0;
  if (k == a.nplanes) { a.block->view_only = (long long)s_sum[0]; return; }
  const long long n_new = (long long)row[4 * (size_t)a.n_rows];
  pps_map_compare_plane p;
  p.n_valid = (long long)s_sum[0] + n_new; p.n_new = n_new;
  const bool any = s_ba[0] >= 1;
  p.best_row = any ? s_br[0] : -1; p.best_plane_id = any ? a.ids[s_br[0]] : -1;
  p.best_n = any ? (long long)s_bn[0] : 0; p.best_agree = any ? (long long)s_ba[0] : 0;
  a.block->planes[k] = p;
}

__global__ __launch_bounds__(kMapThreads) void k_compare_emit(CompareFinishArgs a) {
  __shared__ int s_wave[kMapWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = blockIdx.x;
  const int cols = a.n_rows + 1;
  if (k == a.nplanes) {                                            // the per-row records and the totals
    const unsigned long long* none = a.table + 4 * (size_t)a.nplanes * (size_t)cols;
    for (int r = tid; r < a.n_rows; r += kMapThreads) {
      const long long unseen = (long long)none[4 * (size_t)r];
      long long view = unseen;
      for (int j = 0; j < a.nplanes; j++) view += (long long)a.table[4 * ((size_t)j * (size_t)cols + (size_t)r)];
      a.rows[r] = pps_map_compare_row{view, unseen};
    }
    if (tid == 0) {
      CompareHead h = {0, 0, a.block->view_only, (long long)none[4 * (size_t)a.n_rows], (long long)a.table[4 * compare_entries(a.nplanes, a.n_rows)], 0};
      for (int j = 0; j < a.nplanes; j++) {
        h.n_both += a.block->planes[j].n_valid - a.block->planes[j].n_new;
        h.n_frame_only += a.block->planes[j].n_new;
        h.n_pairs += a.block->pair_cnt[j];
      }
      a.block->head = h;
    }
    return;
  }
  long long run = 0;
  for (int j = 0; j < k; j++) run += a.block->pair_cnt[j];
  const unsigned long long* row = a.table + 4 * (size_t)k * (size_t)cols;
  for (int r0 = 0; r0 < a.n_rows; r0 += kMapThreads) {             // (workgroup-uniform bounds: every thread meets the barriers)
    const int r = r0 + tid;
    unsigned long long e[4] = {0ull, 0ull, 0ull, 0ull};
    if (r < a.n_rows)
      for (int j = 0; j < 4; j++) e[j] = row[4 * (size_t)r + j];
    const bool keep = e[0] > 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kMapWaves; w++) { const int v = s_wave[w]; all += v; if (w < wv) before += v; }
    __syncthreads();
    if (keep)
      a.pairs[run + before + map_lanes_below(m)] = pps_map_compare_pair{k, r, a.ids[r], 0, (long long)e[0], (long long)e[1], (long long)e[2], (long long)e[3]};
    run += all;
  }
}

}  // namespace

hipError_t launch_compare(const CompareArgs& a, hipStream_t st) {
  if (a.npx < 1 || a.nplanes < 1 || a.nplanes > kComparePlanes || a.n_rows < 0) return hipErrorInvalidValue;
  const int per = kComparePasses * kMapThreads;
  hipLaunchKernelGGL(k_compare, dim3((unsigned int)((a.npx + per - 1) / per)), dim3(kMapThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_compare_finish(const CompareFinishArgs& a, hipStream_t st) {
  if (a.nplanes < 1 || a.nplanes > kComparePlanes || a.n_rows < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_compare_scan, dim3((unsigned int)(a.nplanes + 1)), dim3(kMapThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_compare_emit, dim3((unsigned int)(a.nplanes + 1)), dim3(kMapThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace pps
