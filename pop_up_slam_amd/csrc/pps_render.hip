// pps_render.hip -- the grid map seen from a camera pose (include/pps.h: pps_map_render).
//
//   k_render_slots  slot[c] for every box cell c of the last grid: its index in the grid map, -1 if it was not emitted.  The compaction of
//                   k_grid_emit (pps_grid.hip) over the same cnt[] and tile_prefix[], writing the position instead of the point; launched
//                   once per grid, by the first render.
//   k_render        one thread per pixel, workgroups of 256 over tiles of 16 x 16 pixels.  The landmark table passes through LDS in slices of
//                   256 rows (every thread reads the same row: a broadcast); per row the thread intersects its ray with the plane
//                   (pps_render_ray.h, the text the host entry points are compiled from), and only a depth in front of the best hit so far
//                   goes on to the point, its cell and the rings of the slot table.  The slot table answers both questions of a cell --
//                   was it emitted, and where --, so cnt[] is not read here.  Every index into it is checked against the row's box first.
//                   The loops are bounded by the row count and (2 reach + 1)^2; a workgroup waits for no other.  n_hit: one ballot per
//                   wave, one atomic add per workgroup.
//
// Compiled without contraction (Makefile), like pps_grid.hip.
#include <hip/hip_runtime.h>

#include "pps_map_window.h"
#include "pps_render.h"

namespace pps {
namespace {

__global__ __launch_bounds__(kMapThreads) void k_render_slots(long long n_cells_all, unsigned int min_count, const unsigned int* __restrict__ cnt,
                                                              const long long* __restrict__ tile_prefix, long long cpw, int* __restrict__ slot) {
  __shared__ int s_wave[kMapWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long c0 = (long long)blockIdx.x * cpw, c1 = min(n_cells_all, c0 + cpw);
  long long run = tile_prefix[blockIdx.x];
  for (long long b = c0; b < c1; b += kMapThreads) {               // (workgroup-uniform bounds: every thread meets the barriers)
    const long long c = b + tid;
    const bool keep = c < c1 && cnt[c] >= min_count;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < kMapWaves; k++) { const int v = s_wave[k]; all += v; if (k < wv) before += v; }
    __syncthreads();
    if (c < c1) slot[c] = keep ? (int)(run + before + map_lanes_below(m)) : -1;
    run += all;
  }
}

__global__ __launch_bounds__(kMapThreads) void k_render(RenderArgs a, int tiles_x) {
  __shared__ RenderPlane s_rows[kRenderSlice];
  __shared__ int s_wave[kMapWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty = (int)(blockIdx.x / (unsigned int)tiles_x), tx = (int)(blockIdx.x - (unsigned int)ty * (unsigned int)tiles_x);
  const int col = tx * kRenderTile + (tid & (kRenderTile - 1)), row = ty * kRenderTile + tid / kRenderTile;
  const bool inside = col < a.width && row < a.height;
  double o[3], ds[3], dw[3];
  render_ray(a.iK, a.T, col, row, o, ds, dw);
  double best_z = INFINITY;
  float best_x[3] = {0.f, 0.f, 0.f};
  int best_row = -1;
  long long best_cell = -1;
  for (int r0 = 0; r0 < a.n_rows; r0 += kRenderSlice) {            // (workgroup-uniform bounds: every thread meets the barriers)
    const int nr = min(kRenderSlice, a.n_rows - r0);
    __syncthreads();
    if (tid < nr) s_rows[tid] = a.rows[r0 + tid];
    __syncthreads();
    if (!inside) continue;
    for (int r = 0; r < nr; r++) {
      const RenderPlane& pl = s_rows[r];
      double t, z;
      if (!render_depth(o, ds, dw, pl, a.z_near, a.z_far, &t, &z)) continue;
      if (best_row >= 0 && !(z < best_z)) continue;                // (among equal z the earlier row keeps the pixel)
      float xf[3];
      long long ci, cj;
      if (!render_point(o, dw, t, pl, a.inv_cell, xf, &ci, &cj)) continue;
      const int* slot = a.slot;
      const long long s = render_lookup(pl, ci, cj, a.reach, [slot](long long c) { return (long long)slot[c]; });
      if (s < 0) continue;
      best_z = z; best_row = r0 + r; best_cell = s;
      best_x[0] = xf[0]; best_x[1] = xf[1]; best_x[2] = xf[2];
    }
  }
  const bool hit = inside && best_row >= 0;
  if (inside) {
    const size_t px = (size_t)row * (size_t)a.width + (size_t)col;
    MapPt pt = {0.f, 0.f, 0.f, 0u};
    if (hit) { pt.x = best_x[0]; pt.y = best_x[1]; pt.z = best_x[2]; pt.rgba = a.pts[best_cell].rgba; }
    a.cloud[px] = pt;
    a.depth[px] = hit ? (float)best_z : 0.f;
    a.plane_id[px] = hit ? a.ids[best_row] : -1;
    a.cell[px] = best_cell;
  }
  const unsigned long long m = __ballot(hit);
  if (lane == 0) s_wave[wv] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int all = 0;
    for (int k = 0; k < kMapWaves; k++) all += s_wave[k];
    if (all) atomicAdd(a.n_hit, (unsigned long long)all);
  }
}

}  // namespace

hipError_t launch_render_slots(long long n_cells_all, unsigned int min_count, const unsigned int* cnt, const long long* tile_prefix, int* slot,
                               hipStream_t st) {
  if (n_cells_all <= 0) return hipSuccess;
  const GridTiling t = grid_tiling(n_cells_all);
  hipLaunchKernelGGL(k_render_slots, dim3(t.nT), dim3(kMapThreads), 0, st, n_cells_all, min_count, cnt, tile_prefix, t.cpw, slot);
  return hipGetLastError();
}

hipError_t launch_render(const RenderArgs& a, hipStream_t st) {
  if (a.width < 1 || a.height < 1 || a.width > kRenderMaxSide || a.height > kRenderMaxSide || a.reach < 0 || a.reach > kRenderMaxReach || a.n_rows < 0)
    return hipErrorInvalidValue;
  const int tiles_x = (a.width + kRenderTile - 1) / kRenderTile, tiles_y = (a.height + kRenderTile - 1) / kRenderTile;
  hipLaunchKernelGGL(k_render, dim3((unsigned int)(tiles_x * tiles_y)), dim3(kMapThreads), 0, st, a, tiles_x);
  return hipGetLastError();
}

}  // namespace pps
