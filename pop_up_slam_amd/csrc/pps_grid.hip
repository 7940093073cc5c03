// pps_grid.hip -- the grid map on the device: one point per lattice cell of every landmark plane (include/pps.h: pps_map_build_grid).
//
// B, the map k_map_build would write for the selection, is never materialised: each pass walks B's indices, finds a point's chunk in
// k_map_build's chunk window (pps_map_window.h), projects the raw point with project_to_plane_f32 -- B's bits -- and
// computes its cell with grid_cell (pps_grid_cell.h), the text the host entry points are compiled from.
//
//   k_grid_extent   per landmark min / max of i and j, and the points that voted.  Integer atomics after a reduction inside the wave.
//   k_grid_vote     per cell a 64-bit max of a key made from the index in B (NEWEST: index + 1, OLDEST: bias - index; 0 = empty) and an
//                   integer add of 1.  Points of one frame plane come in raster order, so the lanes of a wave that fall into one cell are
//                   mostly neighbours: a run of consecutive lanes with the same cell sends ONE atomic pair (its winner is the run's last
//                   or first lane, its count the run's length).  The key and count arrays are touched by atomics only and read by the
//                   next kernels.
//   k_grid_count / k_grid_scan / k_grid_plane_off / k_grid_emit
//                   the stable compaction of the cells with count >= min_count in cell order -- count per tile, scan over the tiles,
//                   write at tile prefix + rank; no atomic cursor --, and the emitted cells before every landmark.
//
// pps_map_build_grid_posed: the same passes with B the posed map.  The three kernels that form a point of B (extent, vote, emit) do so
// through grid_b_point, which moves the point with its frame's motion first when it is given a motion table (pps_map_move.h).
//
// Max, min and add of integers do not depend on the order they arrive in: two runs give the same bytes.
// Compiled without contraction (Makefile), like pps_map.hip.
#include <hip/hip_runtime.h>

#include <climits>

#include "pps_grid.h"
#include "pps_grid_cell.h"
#include "pps_map_move.h"
#include "pps_map_window.h"
#include "pps_project.h"

namespace pps {
namespace {

constexpr int kGridExtentTurns = 4;     // landmarks reduced inside a wave before the rest of its lanes send their own atomics

typedef MapWindow<true> GridWindow;       // the chunk window of 256 consecutive points of B; its fourth row: the landmark of every chunk

// The point B holds for the stored point *pt of chunk c (a row of the selection; sl: its landmark's slot, -1: gone).  Without a motion
// table B is pps_map_build's: project_to_plane_f32 of the raw point.  With one B is the posed map (pps_map_build_grid_posed): a point of
// a frame that has a motion is moved and then projected (map_moved_point, pps_map_move.h), every other point is formed as before.
__device__ __forceinline__ void grid_b_point(const GridSelArgs& a, const MapMotionTable& mt, int c, int sl, MapPt* pt) {
  double p[4] = {0.0, 0.0, 1.0, 0.0};
  if (sl >= 0)
    for (int k = 0; k < 4; k++) p[k] = a.plane_est[(size_t)k * a.plane_ld + sl];
  if (mt.motion) {
    const int f = mt.fidx[c];
    if (mt.moved[f]) {
      double D[12];
      for (int k = 0; k < 12; k++) D[k] = mt.motion[12 * (size_t)f + k];
      map_moved_point(D, p, sl >= 0, &pt->x, &pt->y, &pt->z);
      return;
    }
  }
  if (sl >= 0) project_to_plane_f32(p, pt->x, pt->y, pt->z, &pt->x, &pt->y, &pt->z);
}

// point i of B (i < n_out): its landmark row (-1: it passes through) and, for a landmark's point, its cell; false if it is dropped
__device__ __forceinline__ bool grid_point_cell(const GridSelArgs& a, const MapMotionTable& mt, const GridWindow& w, long long i, int* lm, long long* ci,
                                                long long* cj) {
  const int lo = map_window_find(w, i);
  const int L = w.aux[lo];
  *lm = L;
  if (L < 0) return true;
  MapPt pt = a.store[w.src[lo] + (i - w.off[lo])];
  grid_b_point(a, mt, w.c0 + lo, w.slot[lo], &pt);
  const GridPlaneDev& pl = a.planes[L];
  const bool oi = grid_cell(pl.e1, a.inv_cell, pt.x, pt.y, pt.z, ci);
  const bool oj = grid_cell(pl.e2, a.inv_cell, pt.x, pt.y, pt.z, cj);
  return oi && oj;
}

__global__ __launch_bounds__(kMapThreads) void k_grid_extent(GridSelArgs a, MapMotionTable mt, GridExtent* __restrict__ ext, unsigned long long* __restrict__ n_dropped) {
  __shared__ GridWindow w;
  const int lane = threadIdx.x & 63;
  const long long first = (long long)blockIdx.x * kMapThreads;
  map_stage_window(w, a.out_off, a.src_off, a.slot, a.lm, a.n_sel, first);
  const long long i = first + threadIdx.x;
  int lm = -1;
  long long ci = 0, cj = 0;
  bool dropped = false;
  if (i < a.n_out && !grid_point_cell(a, mt, w, i, &lm, &ci, &cj)) { dropped = true; lm = -1; }
  const unsigned long long dm = __ballot(dropped);
  if (dm && lane == 0) atomicAdd(n_dropped, (unsigned long long)__popcll(dm));
  const int vi = (int)ci, vj = (int)cj;                          // (|i|, |j| < 2^30)
  unsigned long long rem = __ballot(lm >= 0);
  for (int turn = 0; rem && turn < kGridExtentTurns; turn++) {   // one turn per landmark among the 64 points (wave-uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const int L = __builtin_amdgcn_readlane(lm, leader);
    const bool mine = lm == L;
    const unsigned long long m = __ballot(mine);
    int i_lo = mine ? vi : INT_MAX, i_hi = mine ? vi : INT_MIN, j_lo = mine ? vj : INT_MAX, j_hi = mine ? vj : INT_MIN;
    for (int d = 32; d > 0; d >>= 1) {
      i_lo = min(i_lo, __shfl_xor(i_lo, d)); i_hi = max(i_hi, __shfl_xor(i_hi, d));
      j_lo = min(j_lo, __shfl_xor(j_lo, d)); j_hi = max(j_hi, __shfl_xor(j_hi, d));
    }
    if (lane == leader) {
      atomicMin(&ext[L].imin, i_lo); atomicMax(&ext[L].imax, i_hi);
      atomicMin(&ext[L].jmin, j_lo); atomicMax(&ext[L].jmax, j_hi);
      atomicAdd(&ext[L].n_in, (unsigned long long)__popcll(m));
    }
    rem &= ~m;
  }
  if (lm >= 0 && ((rem >> lane) & 1ull)) {                       // more landmarks in one wave than turns: one-point chunks
    atomicMin(&ext[lm].imin, vi); atomicMax(&ext[lm].imax, vi);
    atomicMin(&ext[lm].jmin, vj); atomicMax(&ext[lm].jmax, vj);
    atomicAdd(&ext[lm].n_in, 1ull);
  }
}

__device__ __forceinline__ unsigned long long grid_key(long long idx, int oldest) {
  return oldest ? kGridOldestBias - (unsigned long long)idx : (unsigned long long)idx + 1ull;
}
__device__ __forceinline__ long long grid_key_index(unsigned long long key, int oldest) {
  return oldest ? (long long)(kGridOldestBias - key) : (long long)(key - 1ull);
}

template <bool COMBINE>
__global__ __launch_bounds__(kMapThreads) void k_grid_vote(GridSelArgs a, MapMotionTable mt, int oldest, unsigned long long* __restrict__ key, unsigned int* __restrict__ cnt) {
  __shared__ GridWindow w;
  const int lane = threadIdx.x & 63;
  const long long first = (long long)blockIdx.x * kMapThreads;
  map_stage_window(w, a.out_off, a.src_off, a.slot, a.lm, a.n_sel, first);
  const long long i = first + threadIdx.x;
  long long c = -1;                                              // the point's cell in the arrays, -1: it does not vote
  if (i < a.n_out) {
    int lm; long long ci, cj;
    if (grid_point_cell(a, mt, w, i, &lm, &ci, &cj) && lm >= 0) {
      const GridPlaneDev& pl = a.planes[lm];
      const long long di = ci - pl.i0, dj = cj - pl.j0;
      if (di >= 0 && di < pl.ni && dj >= 0 && dj < pl.nj) c = pl.base + dj * pl.ni + di;      // (always, after the extent pass; the arrays end at the boxes)
    }
  }
  if (!COMBINE) {
    if (c >= 0) { atomicMax(&key[c], grid_key(i, oldest)); atomicAdd(&cnt[c], 1u); }
    return;
  }
  // runs of consecutive lanes with one cell: the head sends the run's vote
  const unsigned int c_lo = (unsigned int)c, c_hi = (unsigned int)((unsigned long long)c >> 32);
  const unsigned int p_lo = __shfl_up(c_lo, 1), p_hi = __shfl_up(c_hi, 1);
  const bool head = lane == 0 || p_lo != c_lo || p_hi != c_hi;
  const unsigned long long heads = __ballot(head);
  if (head && c >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = above ? __ffsll((long long)above) : 64 - lane;
    const long long win = oldest ? i : i + (len - 1);
    atomicMax(&key[c], grid_key(win, oldest));
    atomicAdd(&cnt[c], (unsigned int)len);
  }
}

// ---- emission ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kMapThreads) void k_grid_count(GridEmitArgs e, long long cpw) {
  __shared__ int s_sum[kMapThreads];
  const int tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * cpw, c1 = min(e.n_cells_all, c0 + cpw);
  int n = 0;
  for (long long c = c0 + tid; c < c1; c += kMapThreads) n += e.cnt[c] >= e.min_count ? 1 : 0;
  const int all = map_block_sum(s_sum, n);
  if (tid == 0) e.tile_count[blockIdx.x] = all;
}

// exclusive scan of the tile counts (one workgroup); tile_prefix[nT] = the sum
__global__ __launch_bounds__(kMapThreads) void k_grid_scan(const int* __restrict__ tile_count, int nT, long long* __restrict__ tile_prefix) {
  __shared__ long long s_sum[kMapThreads];
  const int tid = threadIdx.x;
  const int seg = (nT + kMapThreads - 1) / kMapThreads;
  const int a = (int)min((long long)nT, (long long)tid * seg), b = (int)min((long long)nT, (long long)a + seg);
  long long sum = 0;
  for (int i = a; i < b; i++) sum += tile_count[i];
  const long long upto = map_block_scan(s_sum, sum);
  long long run = upto - sum;
  for (int i = a; i < b; i++) { tile_prefix[i] = run; run += tile_count[i]; }
  if (tid == kMapThreads - 1) tile_prefix[nT] = upto;
}

// emitted cells before the first cell of landmark L (one workgroup per row of plane_base): the prefix of its tile plus the tile's cells before it
__global__ __launch_bounds__(kMapThreads) void k_grid_plane_off(GridEmitArgs e, long long cpw) {
  __shared__ int s_sum[kMapThreads];
  const int tid = threadIdx.x;
  const long long c1 = e.plane_base[blockIdx.x];
  const long long T = c1 / cpw, c0 = T * cpw;
  int n = 0;
  for (long long c = c0 + tid; c < c1; c += kMapThreads) n += e.cnt[c] >= e.min_count ? 1 : 0;
  const int before = map_block_sum(s_sum, n);
  if (tid == 0) e.plane_off[blockIdx.x] = e.tile_prefix[T] + before;
}

__global__ __launch_bounds__(kMapThreads) void k_grid_emit(GridSelArgs a, MapMotionTable mt, GridEmitArgs e, long long cpw) {
  __shared__ int s_wave[kMapWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long c0 = (long long)blockIdx.x * cpw, c1 = min(e.n_cells_all, c0 + cpw);
  long long run = e.tile_prefix[blockIdx.x];
  for (long long b = c0; b < c1; b += kMapThreads) {             // (workgroup-uniform bounds: every thread meets the barriers)
    const long long c = b + tid;
    unsigned int n = 0;
    if (c < c1) n = e.cnt[c];
    const bool keep = c < c1 && n >= e.min_count;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < kMapWaves; k++) { const int v = s_wave[k]; all += v; if (k < wv) before += v; }
    __syncthreads();
    if (keep) {
      const long long pos = run + before + map_lanes_below(m);
      const GridPlaneDev& pl = a.planes[map_find(e.plane_base, a.n_planes, c)];
      const long long rel = c - pl.base;
      const long long dj = rel / pl.ni, di = rel - dj * pl.ni;
      const long long idx = grid_key_index(e.key[c], e.oldest);
      const int lo = map_find(a.out_off, a.n_sel, idx);
      MapPt pt = {0.f, 0.f, 0.f, 0u};
      if (idx >= 0 && idx < a.n_out) {                           // (always: the key of a counted cell is a point's)
        pt = a.store[a.src_off[lo] + (idx - a.out_off[lo])];
        grid_b_point(a, mt, lo, a.slot[lo], &pt);
      }
      e.pts[pos] = pt;
      e.counts[pos] = n;
      e.ij[2 * pos] = pl.i0 + (int)di; e.ij[2 * pos + 1] = pl.j0 + (int)dj;
      e.src[pos] = idx;
    }
    run += all;
  }
}

}  // namespace

hipError_t launch_grid_extent(const GridSelArgs& a, GridExtent* ext, unsigned long long* n_dropped, hipStream_t st, const MapMotionTable& mt) {
  if (a.n_out <= 0 || a.n_sel <= 0) return hipSuccess;
  const long long nwg = (a.n_out + kMapThreads - 1) / kMapThreads;
  if (nwg > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grid_extent, dim3((unsigned int)nwg), dim3(kMapThreads), 0, st, a, mt, ext, n_dropped);
  return hipGetLastError();
}

hipError_t launch_grid_vote(const GridSelArgs& a, int oldest, bool combine, unsigned long long* key, unsigned int* cnt, hipStream_t st,
                            const MapMotionTable& mt) {
  if (a.n_out <= 0 || a.n_sel <= 0) return hipSuccess;
  const long long nwg = (a.n_out + kMapThreads - 1) / kMapThreads;
  if (nwg > 0x7fffffffLL) return hipErrorInvalidValue;
  if (combine) hipLaunchKernelGGL(k_grid_vote<true>, dim3((unsigned int)nwg), dim3(kMapThreads), 0, st, a, mt, oldest, key, cnt);
  else hipLaunchKernelGGL(k_grid_vote<false>, dim3((unsigned int)nwg), dim3(kMapThreads), 0, st, a, mt, oldest, key, cnt);
  return hipGetLastError();
}

hipError_t launch_grid_count(const GridEmitArgs& e, int n_planes, hipStream_t st) {
  if (e.n_cells_all <= 0) return hipSuccess;
  const GridTiling t = grid_tiling(e.n_cells_all);
  hipLaunchKernelGGL(k_grid_count, dim3(t.nT), dim3(kMapThreads), 0, st, e, t.cpw);
  hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(kMapThreads), 0, st, e.tile_count, t.nT, e.tile_prefix);
  hipLaunchKernelGGL(k_grid_plane_off, dim3(n_planes + 1), dim3(kMapThreads), 0, st, e, t.cpw);
  return hipGetLastError();
}

hipError_t launch_grid_emit(const GridSelArgs& a, const GridEmitArgs& e, hipStream_t st, const MapMotionTable& mt) {
  if (e.n_cells_all <= 0) return hipSuccess;
  const GridTiling t = grid_tiling(e.n_cells_all);
  hipLaunchKernelGGL(k_grid_emit, dim3(t.nT), dim3(kMapThreads), 0, st, a, mt, e, t.cpw);
  return hipGetLastError();
}

}  // namespace pps
